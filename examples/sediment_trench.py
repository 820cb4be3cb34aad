#!/usr/bin/env python
"""
Migrating trench: suspended sediment and Exner bed evolution in a flume (after the reference's ``examples/sediment_trench_2d``,
the experiment of Van Rijn 1980).

A 16 m x 1.1 m channel on triangles, 0.397 m deep, with a 0.15 m deep trench between x = 5 and x = 11.5 m whose slopes are 1.5 m long.
Sediment: d50 = 160 um, bed reference height 0.025 m, viscosity 1e-6, porosity 0.4, morphological acceleration factor 100, Nikuradse
roughness 3 d50, sediment diffusivity 0.15.  Inflow: flux -0.22 m^3/s with the sediment at its local equilibrium (``'equilibrium'``);
outflow: elevation 0.  The sediment starts at its equilibrium concentration everywhere.

Differences from the reference: the explicit steppers (SSPRK33 for flow and sediment, one lumped Exner update per step) instead of
CrankNicolson, the suspended load only (no bedload, no slope corrections), ``use_advective_velocity_correction=False``, closures at
the DG nodes.  The script prints the sediment mass at every export and the bed change at the end.

    python examples/sediment_trench.py [--nx 64 --ny 4 --steps 2000 --morfac 100]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import Constant, Function, RectangleMesh, get_functionspace, solver2d     # noqa: E402

LX, LY, DEPTH, TRENCH = 16.0, 1.1, 0.397, 0.15


def trench_bathymetry(x):
    """depth (positive downwards) of the initial bed: 0.397 m, 0.15 m deeper between the two 1.5 m slopes"""
    ramp_in = np.clip((x - 5.0)/1.5, 0.0, 1.0)
    ramp_out = np.clip((11.5 - x)/1.5, 0.0, 1.0)
    return DEPTH + TRENCH*np.minimum(ramp_in, ramp_out)


def setup(argv=None):
    """the solver with its initial conditions assigned, the initial bed and the arguments"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=64)
    ap.add_argument('--ny', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--dt', type=float, default=None, help='time step (default: 0.06 of the shortest edge over the wave speed)')
    ap.add_argument('--morfac', type=float, default=100.0)
    ap.add_argument('--stepper', default='SSPRK33', choices=['SSPRK33', 'ForwardEuler'], help='sediment_timestepper_type')
    args = ap.parse_args(argv)
    mesh2d = RectangleMesh(args.nx, args.ny, LX, LY)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='bathymetry_2d').assign(trench_bathymetry(mesh2d.vertex_xy[:, 0]))
    initial_bed = bathymetry_2d.dat.data_ro.copy()

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    so = options.sediment_model_options
    so.solve_suspended_sediment = True
    so.solve_exner = True
    so.use_advective_velocity_correction = False
    so.average_sediment_size = Constant(160e-6)
    so.bed_reference_height = Constant(0.025)
    so.morphological_acceleration_factor = Constant(args.morfac)
    so.horizontal_diffusivity = Constant(0.15)
    so.check_sediment_conservation = True
    options.horizontal_viscosity = Constant(1e-6)
    options.nikuradse_bed_roughness = Constant(3*160e-6)
    options.no_exports = True
    options.set_timestepper_type('SSPRK33')
    so.sediment_timestepper_type = args.stepper
    for o in (options.swe_timestepper_options, options.tracer_timestepper_options, so.sediment_timestepper_options):
        o.use_automatic_timestep = False
    h = min(LX/args.nx, LY/args.ny)
    # explicit limits: the gravity wave (sqrt(g H) + u ~ 2.9 m/s) and the SIPG diffusion of the sediment (~ h^2/(30 mu))
    dt = args.dt if args.dt is not None else min(0.06*h/2.9, h*h/(30.0*0.15))
    options.timestep = dt
    options.simulation_end_time = args.steps*dt
    options.simulation_export_time = max(1, args.steps//4)*dt

    left, right = 1, 2
    solver_obj.bnd_functions['shallow_water'] = {left: {'flux': Constant(-0.22)}, right: {'elev': Constant(0.0)}}
    solver_obj.bnd_functions['sediment'] = {left: {'equilibrium': None}, right: {}}
    uv_init = Function(get_functionspace(mesh2d, 'DG', 1, vector=True))
    H0 = trench_bathymetry(np.asarray(uv_init.function_space().node_xy())[:, 0])
    uv_init.dat.data[:, 0] = 0.22/LY/H0                       # the inflow's discharge per unit width over the local depth
    solver_obj.assign_initial_conditions(uv=uv_init)
    return solver_obj, initial_bed, args


def main(argv=None):
    solver_obj, initial_bed, args = setup(argv)
    dt = solver_obj.options.timestep
    solver_obj.iterate()

    bed = solver_obj.fields.bathymetry_2d.dat.data_ro
    change = bed - initial_bed                                 # > 0: eroded (deeper), < 0: accreted
    sed = solver_obj.fields.sediment_2d.dat.data_ro
    print('steps {:d}  dt {:.5f}  t {:.3f} s  (morphological time {:.1f} s)'.format(solver_obj.iteration, dt, solver_obj.simulation_time,
                                                                                   args.morfac*solver_obj.simulation_time))
    print('sediment {:.4e} ... {:.4e}'.format(sed.min(), sed.max()))
    print('bed change {:+.4e} ... {:+.4e} m'.format(change.min(), change.max()))
    assert np.isfinite(bed).all() and np.isfinite(sed).all()
    solver_obj.bed_change = change
    return solver_obj


if __name__ == '__main__':
    main()
