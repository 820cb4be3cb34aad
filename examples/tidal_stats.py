#!/usr/bin/env python
"""
Co-tidal chart of a tidal channel: the open end (boundary 1, x = 0) follows an M2 tide with an M4 overtide, and a
``FieldStatisticsCallback`` accumulates - on the device, every tenth step, without leaving the batched ``iterate()`` - the extrema and
means of the fields and the harmonic sums of the elevation at every node.  After two M2 periods the least-squares fit gives the M2 /
M4 amplitude and phase everywhere, next to the maximum speed, the residual current and the mean of |u|^3.

    python examples/tidal_stats.py [--nx 16 --ny 4 --periods 2 --every 10]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, FieldStatisticsCallback, Function, HarmonicTidalForcing, RectangleMesh,           # noqa: E402
                        get_functionspace, solver2d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=16)
    ap.add_argument('--ny', type=int, default=4)
    ap.add_argument('--periods', type=float, default=2.0, help='length of the run in M2 periods')
    ap.add_argument('--every', type=int, default=10, help='sample every n-th step')
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
    options.quadratic_drag_coefficient = Constant(0.0025)

    y = P1_2d.node_xy()[:, 1]
    tide = HarmonicTidalForcing(Function(P1_2d, name='tidal_elev'), [m2, 2*m2],
                                np.stack([0.8 + 0.0*y, 0.1 + 0.0*y]), np.stack([0.0*y, 0.7 + 0.0*y]), mean=0.0)
    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': tide}}
    solver_obj.assign_initial_conditions(elev=Constant(0.0))
    # the first half period is spin-up from rest: sampled from there on
    stats = FieldStatisticsCallback(solver_obj, harmonics={'M2': m2, 'M4': 2*m2}, every=args.every, start_time=math.pi/m2,
                                    export_to_hdf5=False)
    solver_obj.add_callback(stats, 'timestep')
    solver_obj.iterate()

    r = stats.result()
    print('steps {:d}  samples {:d}  cond(W) {:.2f}'.format(solver_obj.iteration, stats.n_samples, float(np.linalg.cond(stats.W))))
    print('M2 amplitude {:.4f} ... {:.4f} m   M4 amplitude {:.4f} ... {:.4f} m'.format(
        r['elev_amp']['M2'].min(), r['elev_amp']['M2'].max(), r['elev_amp']['M4'].min(), r['elev_amp']['M4'].max()))
    print('elevation {:.4f} ... {:.4f} m   max speed {:.4f} m/s   mean |u|^3 up to {:.4e} m3/s3   residual current up to {:.4e} m/s'.format(
        r['elev_min'].min(), r['elev_max'].max(), r['speed_max'].max(), r['speed_cubed_mean'].max(),
        np.hypot(r['uv_mean'][:, 0], r['uv_mean'][:, 1]).max()))


if __name__ == '__main__':
    main()
