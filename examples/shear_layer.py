#!/usr/bin/env python
"""
Two opposed streams in a closed channel (walls all round, no periodic direction): a shear layer along the channel's axis, with the
Smagorinsky eddy viscosity (options.use_smagorinsky_viscosity) evaluated on the device in front of every step.  The closure answers
the strain: it is large inside the shear band and stays near its floor in the two streams.

    python examples/shear_layer.py [--nx 48 --ny 24 --t-end 120 --export]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import Constant, Function, RectangleMesh, get_functionspace, solver2d       # noqa: E402


def run(nx=48, ny=24, t_end=120.0, export=False, output_directory='outputs'):
    lx, ly = 20e3, 10e3
    u0, width = 0.5, 0.1*ly                                   # stream speed, half-width of the shear band
    mesh2d = RectangleMesh(nx, ny, lx, ly)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').assign(20.0)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    options.swe_timestepper_type = 'SSPRK33'
    options.horizontal_velocity_scale = Constant(2.0*u0)      # used by the automatic CFL time step
    options.simulation_export_time = t_end
    options.simulation_end_time = t_end
    options.horizontal_viscosity = Constant(1.0)              # the background the closure is added to
    options.use_smagorinsky_viscosity = True
    options.smagorinsky_coefficient = Constant(0.2)
    options.fields_to_export = ['uv_2d', 'elev_2d', 'smag_visc_2d']
    options.no_exports = not export
    options.output_directory = output_directory

    # u = u0 tanh((y - ly/2)/width), with a small meander that the layer rolls up from
    P1v_2d = get_functionspace(mesh2d, 'CG', 1, vector=True)
    uv_init = Function(P1v_2d).interpolate(lambda x, y: (u0*np.tanh((y - 0.5*ly)/width)*np.sin(np.pi*x/lx)**2,
                                                         0.02*u0*np.sin(4*np.pi*x/lx)*np.exp(-((y - 0.5*ly)/width)**2)))
    solver_obj.assign_initial_conditions(uv=uv_init)
    solver_obj.iterate()

    nu = solver_obj.fields.smag_visc_2d.dat.data_ro
    y = mesh2d.vertex_xy[:, 1]
    band = np.abs(y - 0.5*ly) <= width
    inside, outside = float(nu[band].max()), float(nu[~band & (np.abs(y - 0.5*ly) > 2.5*width)].max())
    print('smag_visc_2d: max inside the shear band {:.4e} m2/s, outside {:.4e} m2/s'.format(inside, outside))
    return inside, outside, solver_obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=48)
    ap.add_argument('--ny', type=int, default=24)
    ap.add_argument('--t-end', type=float, default=120.0)
    ap.add_argument('--export', action='store_true', help='write VTK files to outputs/')
    args = ap.parse_args()
    run(args.nx, args.ny, args.t_end, args.export)


if __name__ == '__main__':
    main()
