#!/usr/bin/env python
"""
Tidal farm in a rectangular channel: the forward half of the reference's examples/tidalfarm/tidalfarm.py written against
thetis_amd.  A sinusoidal tide is imposed as 'elev' on both open ends (through ``update_forcings``), the channel has a
quadratic bottom drag, and a farm of constant-thrust turbines with a uniform density fills the subdomain in its middle, which
the mesh marks with ``cell_marker_fn`` (the reference reads the subdomain id from headland.msh).  The performance of the farm is
followed by ``TurbineFunctionalCallback``; its line is printed at every export and once more at the end.

    python examples/tidalfarm.py [--nx 40 --ny 10 --t-end 3600]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, Function, RectangleMesh, TidalTurbineFarmOptions, get_functionspace, solver2d,    # noqa: E402
                        turbines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=40)
    ap.add_argument('--ny', type=int, default=10)
    ap.add_argument('--t-end', type=float, default=3600.0)
    ap.add_argument('--export', action='store_true', help='write VTK files to outputs/')
    args = ap.parse_args()
    lx, ly, site_id = 20e3, 5e3, 2
    mesh2d = RectangleMesh(args.nx, args.ny, lx, ly,
                           cell_marker_fn=lambda x, y: np.where((abs(x - lx/2) < 1.5e3) & (abs(y - ly/2) < 1e3), site_id, 0))
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').assign(50.0)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    options.timestep = 2.0                                   # explicit: below the gravity-wave limit of the 500 m cells
    options.simulation_export_time = 600.0
    options.simulation_end_time = args.t_end
    options.output_directory = 'outputs'
    options.check_volume_conservation_2d = False
    options.element_family = 'dg-dg'
    options.swe_timestepper_type = 'SSPRK33'
    options.swe_timestepper_options.use_automatic_timestep = False
    options.fields_to_export = ['uv_2d', 'elev_2d']
    options.no_exports = not args.export
    options.quadratic_drag_coefficient = Constant(0.0025)

    # the farm: constant-thrust turbines (C_T = 0.8, D = 18 m), uniform density in the site
    farm_options = TidalTurbineFarmOptions()
    farm_options.turbine_density = Constant(5e-5)             # turbines per m^2
    farm_options.turbine_options.diameter = 18.0
    farm_options.turbine_options.thrust_coefficient = 0.8
    farm_options.break_even_wattage = 5e4
    options.tidal_turbine_farms[site_id] = [farm_options]

    # tidal elevation on the open ends, half a period apart
    t_tide, amp = 12.42*3600.0, 0.8
    left, right = Constant(0.0), Constant(0.0)
    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': left}, 2: {'elev': right}}

    def update_forcings(t):
        left.assign(amp*math.sin(2*math.pi*t/t_tide + 0.5*math.pi))
        right.assign(-amp*math.sin(2*math.pi*t/t_tide + 0.5*math.pi))

    update_forcings(0.0)
    solver_obj.create_equations()
    cb = turbines.TurbineFunctionalCallback(solver_obj)
    solver_obj.add_callback(cb, 'export')
    solver_obj.assign_initial_conditions(elev=lambda x, y: amp*(1 - 2*x/lx), uv=Constant((0.5, 0.0)))
    solver_obj.iterate(update_forcings=update_forcings)
    print(cb.message_str(*cb()))
    print('turbines {:.3f} average_power_W {:.6e}'.format(sum(cb.cost), sum(cb.average_power)))


if __name__ == '__main__':
    main()
