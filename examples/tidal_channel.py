#!/usr/bin/env python
"""
Tidal channel: a rectangular channel whose open end (boundary 1, x = 0) follows an M2 + S2 tide.  The tide is a
``HarmonicTidalForcing`` given itself as the boundary's 'elev': the device evaluates the two constituents in front of every
Runge-Kutta stage, and the plain ``iterate()`` below - no ``update_forcings`` - issues all steps between two exports in one call
into the library.  A detector in mid-channel takes a row at every time step on the way (``DetectorsCallback``); ``--farm`` adds a
farm of constant-thrust turbines in the middle of the channel.

    python examples/tidal_channel.py [--nx 16 --ny 4 --t-end 600 --farm]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, DetectorsCallback, Function, HarmonicTidalForcing, RectangleMesh,           # noqa: E402
                        TidalTurbineFarmOptions, get_functionspace, solver2d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--ny', type=int, default=4)
    ap.add_argument('--t-end', type=float, default=600.0)
    ap.add_argument('--farm', action='store_true', help='a turbine farm in the middle of the channel')
    ap.add_argument('--export', action='store_true', help='write VTK files to outputs/')
    args = ap.parse_args()
    lx, ly, site_id = 40e3, 10e3, 2
    mesh2d = RectangleMesh(args.nx, args.ny, lx, ly,
                           cell_marker_fn=lambda x, y: np.where((abs(x - lx/2) < 5e3) & (abs(y - ly/2) < 2.5e3), site_id, 0))
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').interpolate(lambda x, y: 40.0 - 10.0*x/lx)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    dx = min(lx/args.nx, ly/args.ny)
    options.timestep = 0.1*dx/math.sqrt(9.81*40.0)            # explicit: well below the gravity-wave limit
    options.simulation_export_time = 20*options.timestep
    options.simulation_end_time = args.t_end
    options.output_directory = 'outputs'
    options.element_family = 'dg-dg'
    options.swe_timestepper_type = 'SSPRK33'
    options.swe_timestepper_options.use_automatic_timestep = False
    options.fields_to_export = ['uv_2d', 'elev_2d']
    options.no_exports = not args.export
    options.quadratic_drag_coefficient = Constant(0.0025)
    if args.farm:
        farm_options = TidalTurbineFarmOptions()
        farm_options.turbine_density = Constant(2e-5)
        farm_options.turbine_options.diameter = 18.0
        farm_options.turbine_options.thrust_coefficient = 0.8
        options.tidal_turbine_farms[site_id] = [farm_options]

    # M2 + S2 on the open end: amplitude and phase vary along the boundary (a Kelvin-wave like tilt)
    y = P1_2d.node_xy()[:, 1]
    omegas = [2*math.pi/(12.4206012*3600.0), 2*math.pi/(12.0*3600.0)]
    amplitudes = np.stack([0.8*(1.0 + 0.1*y/ly), 0.3*(1.0 + 0.1*y/ly)])
    phases = np.stack([0.2*y/ly, 0.7 + 0.2*y/ly])
    tide = HarmonicTidalForcing(Function(P1_2d, name='tidal_elev'), omegas, amplitudes, phases, mean=0.0)
    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': tide}}
    solver_obj.assign_initial_conditions(elev=Constant(0.0))
    gauge = DetectorsCallback(solver_obj, [(lx/2, ly/2)], ['elev_2d', 'uv_2d'], name='gauge', detector_names=['mid'])
    solver_obj.add_callback(gauge, 'timestep')
    solver_obj.iterate()

    d = solver_obj.timestepper.diagnostics()
    print('steps {:d}  time {:.2f}  eta norm {:.6e}  u norm {:.6e}'.format(
        solver_obj.iteration, solver_obj.simulation_time, math.sqrt(d[0]), math.sqrt(d[1])))
    print('gauge rows {:d}  last elevation {:.6e}'.format(len(gauge.history), float(np.ravel(gauge.history[-1][1])[0])))


if __name__ == '__main__':
    main()
