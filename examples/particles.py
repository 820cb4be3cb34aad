#!/usr/bin/env python
"""
Tidal excursion in a channel: the open end (boundary 1, x = 0) follows an M2 tide that the device evaluates itself, and a
``ParticleTrackerCallback`` advects a line of drifters across the channel - on the device, every tenth step, without leaving the
batched ``iterate()``.  After the run the script prints how far the drifters travelled (the largest distance from the release
point along the recorded tracks, and where they ended), how many left through the open end or touched a wall, and writes
``diagnostic_drifters.npz`` with the tracks.

    python examples/particles.py [--nx 16 --ny 4 --periods 1 --every 10 --particles 21 --outdir outputs]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, Function, HarmonicTidalForcing, ParticleTrackerCallback, RectangleMesh,           # noqa: E402
                        get_functionspace, solver2d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--ny', type=int, default=4)
    ap.add_argument('--periods', type=float, default=1.0, help='length of the run in M2 periods')
    ap.add_argument('--every', type=int, default=10, help='move the particles every n-th step')
    ap.add_argument('--particles', type=int, default=21)
    ap.add_argument('--outdir', default='outputs')
    args = ap.parse_args()
    lx, ly = 40e3, 10e3
    mesh2d = RectangleMesh(args.nx, args.ny, lx, ly)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').interpolate(lambda x, y: 40.0 - 10.0*x/lx)

    m2 = 2*math.pi/(12.4206012*3600.0)
    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    dx = min(lx/args.nx, ly/args.ny)
    options.timestep = 0.04*dx/math.sqrt(9.81*40.0)            # explicit, well inside the gravity-wave limit of the triangles
    options.simulation_export_time = 1000*options.timestep
    options.simulation_end_time = args.periods*2*math.pi/m2
    options.swe_timestepper_type = 'SSPRK33'
    options.swe_timestepper_options.use_automatic_timestep = False
    options.no_exports = True
    options.output_directory = args.outdir
    options.quadratic_drag_coefficient = Constant(0.0025)

    y = P1_2d.node_xy()[:, 1]
    tide = HarmonicTidalForcing(Function(P1_2d, name='tidal_elev'), [m2], np.stack([0.8 + 0.0*y]), np.stack([0.0*y]), mean=0.0)
    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': tide}}
    solver_obj.assign_initial_conditions(elev=Constant(0.0))
    # a line of drifters across the channel, a quarter of its length from the open end
    release = np.stack([np.full(args.particles, 0.25*lx), np.linspace(0.05*ly, 0.95*ly, args.particles)], axis=1)
    drifters = ParticleTrackerCallback(solver_obj, release, name='drifters', every=args.every, record_every=10, open_boundaries=(1,))
    solver_obj.add_callback(drifters, 'timestep')
    solver_obj.iterate()

    t, tracks = drifters.trajectories()
    status = drifters.status()
    reach = np.hypot(*(tracks - release[None]).transpose(2, 0, 1)).max(axis=0) if len(tracks) else np.zeros(len(release))
    print('steps {:d}  moves {:d}  rows {:d}'.format(solver_obj.iteration, drifters.n_advances, len(t)))
    print('tidal excursion {:.1f} ... {:.1f} m   final distance from release {:.1f} ... {:.1f} m'.format(
        reach.min(), reach.max(), drifters.excursion().min(), drifters.excursion().max()))
    print('active {:d}  exited {:d}  lost {:d}  wall hits {:d}'.format(int((status == 0).sum()), int((status == 1).sum()),
                                                                      int((status == 2).sum()), int(drifters.wall_hits().sum())))
    drifters.export()
    print('tracks written to', os.path.join(args.outdir, 'diagnostic_drifters.npz'))


if __name__ == '__main__':
    main()
