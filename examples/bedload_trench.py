#!/usr/bin/env python
"""
Migrating trench with suspended load AND bedload (after the reference's ``examples/sediment_trench_2d``, the experiment of Van Rijn
1980), and, with ``--bedload-only``, a hump in a uniform channel moved by the bedload alone.

The trench: the 16 m x 1.1 m channel of ``examples/sediment_trench.py`` with the same sediment, boundaries and steppers, plus
``use_bedload`` with the slope magnitude and slope angle corrections (the reference's defaults).  The bedload transport leaves
through both ends: the inflow carries a flux and the outflow an elevation, neither of which closes a boundary.

``--bedload-only``: ``solve_suspended_sediment = False``; a Gaussian hump 0.1 m high at x = 6 m in a channel 0.4 m deep, discharge
0.26 m^2/s per unit width.  The flow speeds up over the hump, the transport grows up its upstream face and falls down its lee face: the
upstream face erodes, the lee face accretes, the hump travels downstream.

Differences from the reference: the explicit steppers and one lumped, explicit Exner update per step instead of CrankNicolson,
``use_advective_velocity_correction=False``, closures at the DG nodes.  The script prints the bed change and the hump's centroid.

    python examples/bedload_trench.py [--bedload-only] [--nx 64 --ny 4 --steps 2000 --morfac 100]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import Constant, Function, RectangleMesh, get_functionspace, solver2d     # noqa: E402

LX, LY, DEPTH, TRENCH = 16.0, 1.1, 0.397, 0.15
HUMP_DEPTH, HUMP, HUMP_X, HUMP_W, HUMP_Q = 0.4, 0.1, 6.0, 1.2, 0.26


def trench_bathymetry(x):
    """depth (positive downwards) of the initial bed: 0.397 m, 0.15 m deeper between the two 1.5 m slopes"""
    ramp_in = np.clip((x - 5.0)/1.5, 0.0, 1.0)
    ramp_out = np.clip((11.5 - x)/1.5, 0.0, 1.0)
    return DEPTH + TRENCH*np.minimum(ramp_in, ramp_out)


def hump_bathymetry(x):
    return HUMP_DEPTH - HUMP*np.exp(-((x - HUMP_X)/HUMP_W)**2)


def centroid(x, bed):
    """x of the centre of the bed's rise above the channel floor"""
    rise = HUMP_DEPTH - bed
    return float((rise*x).sum()/rise.sum())


def setup(argv=None):
    """the solver with its initial conditions assigned, the initial bed and the arguments"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--bedload-only', action='store_true', help='a hump in a uniform channel, no suspended load')
    ap.add_argument('--nx', type=int, default=64)
    ap.add_argument('--ny', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--dt', type=float, default=None, help='time step (default: 0.06 of the shortest edge over the wave speed)')
    ap.add_argument('--morfac', type=float, default=100.0)
    ap.add_argument('--stepper', default='SSPRK33', choices=['SSPRK33', 'ForwardEuler'], help='sediment_timestepper_type')
    args = ap.parse_args(argv)
    mesh2d = RectangleMesh(args.nx, args.ny, LX, LY)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bed_of = hump_bathymetry if args.bedload_only else trench_bathymetry
    bathymetry_2d = Function(P1_2d, name='bathymetry_2d').assign(bed_of(mesh2d.vertex_xy[:, 0]))
    initial_bed = bathymetry_2d.dat.data_ro.copy()

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    so = options.sediment_model_options
    so.solve_suspended_sediment = not args.bedload_only
    so.solve_exner = True
    so.use_bedload = True
    so.use_angle_correction = True
    so.use_slope_mag_correction = True
    so.use_advective_velocity_correction = False
    so.average_sediment_size = Constant(160e-6)
    so.bed_reference_height = Constant(0.025)
    so.morphological_acceleration_factor = Constant(args.morfac)
    if not args.bedload_only:
        so.horizontal_diffusivity = Constant(0.15)
        so.check_sediment_conservation = True
    options.horizontal_viscosity = Constant(1e-6)
    options.nikuradse_bed_roughness = Constant(3*160e-6)
    options.no_exports = True
    options.set_timestepper_type('SSPRK33')
    so.sediment_timestepper_type = args.stepper
    so.exner_timestepper_type = 'SSPRK33'
    for o in (options.swe_timestepper_options, options.tracer_timestepper_options, so.sediment_timestepper_options):
        o.use_automatic_timestep = False
    h = min(LX/args.nx, LY/args.ny)
    # explicit limits: the gravity wave (sqrt(g H) + u ~ 2.9 m/s) and the SIPG diffusion of the sediment (~ h^2/(30 mu))
    dt = args.dt if args.dt is not None else min(0.06*h/2.9, h*h/(30.0*0.15))
    options.timestep = dt
    options.simulation_end_time = args.steps*dt
    options.simulation_export_time = max(1, args.steps//4)*dt

    left, right = 1, 2
    discharge = HUMP_Q*LY if args.bedload_only else 0.22
    solver_obj.bnd_functions['shallow_water'] = {left: {'flux': Constant(-discharge)}, right: {'elev': Constant(0.0)}}
    if not args.bedload_only:
        solver_obj.bnd_functions['sediment'] = {left: {'equilibrium': None}, right: {}}
    uv_init = Function(get_functionspace(mesh2d, 'DG', 1, vector=True))
    H0 = bed_of(np.asarray(uv_init.function_space().node_xy())[:, 0])
    uv_init.dat.data[:, 0] = discharge/LY/H0                  # the inflow's discharge per unit width over the local depth
    solver_obj.assign_initial_conditions(uv=uv_init)
    return solver_obj, initial_bed, args


def main(argv=None):
    solver_obj, initial_bed, args = setup(argv)
    dt = solver_obj.options.timestep
    solver_obj.iterate()

    bed = solver_obj.fields.bathymetry_2d.dat.data_ro
    change = bed - initial_bed                                 # > 0: eroded (deeper), < 0: accreted
    qbx, qby = solver_obj.sediment_model.get_bedload_term()
    print('steps {:d}  dt {:.5f}  t {:.3f} s  (morphological time {:.1f} s)'.format(solver_obj.iteration, dt, solver_obj.simulation_time,
                                                                                   args.morfac*solver_obj.simulation_time))
    print('bedload transport {:.4e} ... {:.4e} m^2/s'.format(qbx.min(), qbx.max()))
    print('bed change {:+.4e} ... {:+.4e} m'.format(change.min(), change.max()))
    assert np.isfinite(bed).all() and np.isfinite(qbx).all() and np.isfinite(qby).all()
    if args.bedload_only:
        x = solver_obj.mesh2d.vertex_xy[:, 0]
        solver_obj.centroids = (centroid(x, initial_bed), centroid(x, bed))
        print('hump centroid {:.4f} -> {:.4f} m'.format(*solver_obj.centroids))
    else:
        sed = solver_obj.fields.sediment_2d.dat.data_ro
        print('sediment {:.4e} ... {:.4e}'.format(sed.min(), sed.max()))
        assert np.isfinite(sed).all()
    solver_obj.bed_change = change
    return solver_obj


if __name__ == '__main__':
    main()
