#!/usr/bin/env python
"""
A continuous release in the tidal channel of ``examples/particles.py``: particles leave one point at a steady rate over the run
(``release_times``), are carried by the M2 tide and spread by a random walk (``diffusivity``), all on the device and inside the
batched ``iterate()``.  At the end the cloud is turned back into a concentration (``cell_counts`` / ``concentration``: particles per
square metre, scaled here by the mass one particle stands for) and the script prints its maximum and where it lies.

    python examples/particle_plume.py [--nx 16 --ny 8 --periods 0.25 --every 10 --particles 2000 --diffusivity 5 --load 1.0]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, Function, HarmonicTidalForcing, ParticleTrackerCallback, RectangleMesh,           # noqa: E402
                        get_functionspace, solver2d)
from thetis_amd.particles import ACTIVE, EXITED, LOST, WAITING                                                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--ny', type=int, default=8)
    ap.add_argument('--periods', type=float, default=0.25, help='length of the run in M2 periods')
    ap.add_argument('--every', type=int, default=10, help='move the particles every n-th step')
    ap.add_argument('--particles', type=int, default=2000)
    ap.add_argument('--diffusivity', type=float, default=5.0, help='horizontal diffusivity of the random walk, m2/s')
    ap.add_argument('--load', type=float, default=1.0, help='kg/s discharged at the outfall')
    ap.add_argument('--seed', type=int, default=1)
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
    # the outfall: one point a quarter of the channel from the open end, a particle every t_end/N seconds
    t_end = options.simulation_end_time
    outfall = np.tile([[0.25*lx + 13.0, 0.5*ly + 7.0]], (args.particles, 1))
    release_times = t_end*np.arange(args.particles)/args.particles
    plume = ParticleTrackerCallback(solver_obj, outfall, name='plume', every=args.every, record_every=10**9, open_boundaries=(1,),
                                    diffusivity=Constant(args.diffusivity), seed=args.seed, release_times=release_times,
                                    export_to_hdf5=False)
    solver_obj.add_callback(plume, 'timestep')
    solver_obj.iterate()

    status = plume.status()
    counts = plume.cell_counts()
    kg_per_particle = args.load*t_end/args.particles
    conc = plume.concentration().dat.data_ro*kg_per_particle                   # kg/m2 (divide by the depth for kg/m3)
    k = int(np.argmax(conc))
    centre = mesh2d.cell_xy()[k].mean(axis=0)
    print('steps {:d}  moves {:d}  cells {:d}'.format(solver_obj.iteration, plume.n_advances, mesh2d.num_cells))
    print('active {:d}  waiting {:d}  exited {:d}  lost {:d}  wall hits {:d}'.format(
        int((status == ACTIVE).sum()), int((status == WAITING).sum()), int((status == EXITED).sum()), int((status == LOST).sum()),
        int(plume.wall_hits().sum())))
    print('particles counted {:d} in {:d} cells'.format(int(counts.sum()), int((counts > 0).sum())))
    print('concentration maximum {:.6e} kg/m2 in cell {:d} at ({:.0f}, {:.0f}) m, {:.0f} m from the outfall'.format(
        float(conc[k]), k, centre[0], centre[1], float(np.hypot(*(centre - outfall[0])))))


if __name__ == '__main__':
    main()
