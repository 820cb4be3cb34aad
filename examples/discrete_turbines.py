#!/usr/bin/env python
"""
Discrete turbines in a rectangular channel: the set-up of the reference's examples/discrete_turbines/tidal_array.py written
against thetis_amd.  A channel with a quadratic bottom drag and a horizontal viscosity is driven by an elevation difference between
its open ends.  A marked subdomain in its middle holds two discrete farms: three constant-thrust turbines in a row, and six turbines
in two staggered rows with a tabulated thrust curve, the drag of their support structures and the upwind velocity correction.  Each
turbine is a bump density of the radius of its projected diameter; the drag runs as a pass of its own after every stage on the
device, the power is integrated per farm (``TurbineFunctionalCallback``) and per turbine (``farm.turbine_powers()``) at every
time step.  At the end the energy of every turbine is printed, and per farm the identity

    energy of the farm = sum of the energies of its turbines

which holds to rounding, overlapping bumps included.

    python examples/discrete_turbines.py [--nx 60 --ny 20 --t-end 1800]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, DiscreteTidalTurbineFarmOptions, Function, RectangleMesh, get_functionspace, solver2d,    # noqa: E402
                        turbines)
from thetis_amd.callback import DiagnosticCallback                                                                         # noqa: E402


class TurbineEnergyCallback(DiagnosticCallback):
    """integrates the power of every turbine of the discrete farms over the time steps"""
    name = 'turbine_energy'

    def __init__(self, solver_obj, **kwargs):
        super().__init__(solver_obj, **kwargs)
        self.farms = solver_obj.tidal_farms
        self.energy = [np.zeros(len(farm.coordinates)) for farm in self.farms]

    def __call__(self):
        dt = self.solver_obj.options.timestep
        for e, farm in zip(self.energy, self.farms):
            e += farm.turbine_powers()*dt
        return tuple(float(e.sum()) for e in self.energy)

    def message_str(self, *values):
        return 'Energy of the turbines of each farm: {}'.format(list(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=60)
    ap.add_argument('--ny', type=int, default=20)
    ap.add_argument('--t-end', type=float, default=1800.0)
    ap.add_argument('--export', action='store_true', help='write VTK files to outputs/')
    args = ap.parse_args()
    lx, ly, site_id = 3e3, 1e3, 2
    mesh2d = RectangleMesh(args.nx, args.ny, lx, ly,
                           cell_marker_fn=lambda x, y: np.where((abs(x - lx/2) < 600.0) & (abs(y - ly/2) < 350.0), site_id, 0))
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').assign(40.0)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    options.timestep = 0.04*min(lx/args.nx, ly/args.ny)/np.sqrt(9.81*40.0)     # explicit: well below the gravity-wave limit of the cells
    options.simulation_export_time = 300.0
    options.simulation_end_time = args.t_end
    options.output_directory = 'outputs'
    options.swe_timestepper_type = 'SSPRK33'
    options.swe_timestepper_options.use_automatic_timestep = False
    options.fields_to_export = ['uv_2d', 'elev_2d']
    options.no_exports = not args.export
    options.quadratic_drag_coefficient = Constant(0.0025)
    options.horizontal_viscosity = Constant(1.0)

    # three turbines in a row across the channel, constant thrust
    row = DiscreteTidalTurbineFarmOptions()
    row.turbine_type = 'constant'
    row.turbine_options.diameter = 20.0
    row.turbine_options.projected_diameter = 160.0           # the bumps span three cells of the default mesh
    row.turbine_options.thrust_coefficient = 0.8
    row.upwind_correction = False
    row.turbine_coordinates = [[1200.0, y] for y in (300.0, 500.0, 700.0)]
    # six in two staggered rows: thrust table, support drag, upwind correction; the bumps of neighbours overlap
    array = DiscreteTidalTurbineFarmOptions()
    array.turbine_type = 'table'
    array.turbine_options.diameter = 20.0
    array.turbine_options.projected_diameter = 160.0
    array.turbine_options.thrust_speeds = [0.3, 0.5, 2.0, 3.5, 4.0]
    array.turbine_options.thrust_coefficients = [0.05, 0.8, 0.8, 0.4, 0.05]
    array.turbine_options.C_support = 0.7
    array.turbine_options.A_support = 30.0
    array.upwind_correction = True
    array.break_even_wattage = 1e4
    array.turbine_coordinates = [[Constant(1600.0), Constant(y)] for y in (280.0, 500.0, 720.0)] + [[1760.0, y] for y in (390.0, 500.0, 610.0)]
    options.discrete_tidal_turbine_farms[site_id] = [row, array]

    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.15)}, 2: {'elev': Constant(-0.15)}}
    solver_obj.create_equations()
    cb = turbines.TurbineFunctionalCallback(solver_obj, append_to_log=False)
    solver_obj.add_callback(cb, 'timestep')
    each = TurbineEnergyCallback(solver_obj, append_to_log=False)
    solver_obj.add_callback(each, 'timestep')
    solver_obj.assign_initial_conditions(elev=lambda x, y: 0.15*(1 - 2*x/lx), uv=Constant((1.5, 0.0)))
    solver_obj.iterate()

    print(cb.message_str(*cb.history[-1][1:]))
    for i, farm in enumerate(solver_obj.tidal_farms):
        print('farm {:d} number_of_turbines {:.4f} energy {:.9e} J, of its turbines {:.9e} J'.format(
            i, cb.cost[i], cb.integrated_power[i], float(each.energy[i].sum())))
        for j, (xy, e) in enumerate(zip(farm.coordinates, each.energy[i])):
            print('  turbine {:d} at ({:.0f}, {:.0f}) energy {:.6e} J'.format(j, xy[0], xy[1], e))


if __name__ == '__main__':
    main()
