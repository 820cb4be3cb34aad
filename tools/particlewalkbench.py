"""ms per move of a particle set on the device (csrc/swe2d_particles.hip), three ways on the same mesh, state and release points:
(old)   swe2d_particles_advance: swe_particle_kernel, the instance of a set without dispersion or timed releases;
(plain) swe2d_particles_advance_at on a set without either: the same instance through the new entry point;
(walk)  swe2d_particles_advance_at with a diffusivity: the midpoint move, ten Philox rounds and the second walk in one launch
        (steps of about ``--step`` of a cell size); (both) the same with release times that have all passed.
Each burst is ``--advances`` launches back to back between two synchronisations, timed by the host clock; the cases alternate
inside every repeat, and the median and the spread (min ... max) over the repeats are reported.

    python tools/particlewalkbench.py [--nx 707 --ny 707] [--particles 1000000] [--advances 300] [--repeats 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from particlebench import make_solver, release  # noqa: E402
from thetis_amd.pointeval import PointLocator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--particles', type=int, default=1000000)
    ap.add_argument('--advances', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--step', type=float, default=0.2, help='sqrt(6 K dt_move) over the cell size')
    args = ap.parse_args()
    s, lx, ly = make_solver(args.nx, args.ny)
    dev = s.timestepper.device
    dev.advance(50)
    xy = release(args.particles, lx, ly)
    cells = PointLocator(s.mesh2d, xy).cells
    dt_move = 10*s.options.timestep
    K = (args.step*lx/args.nx)**2/(6.0*dt_move)
    sets = {c: dev.particles_create(xy, cells) for c in ('old', 'plain', 'walk', 'both')}
    for c in ('walk', 'both'):
        dev.particles_set_diffusivity(sets[c], K, 1)
    dev.particles_set_release_times(sets['both'], np.zeros(args.particles), 0.0)

    def burst(c, n):
        dev.synchronize()
        t0 = time.perf_counter()
        for j in range(n):
            if c == 'old':
                dev.particles_advance(sets[c], dt_move, (1,))
            else:
                dev.particles_advance_at(sets[c], dt_move, dt_move*(j + 1), (1,))
        dev.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    ms = {c: [] for c in sets}
    for c in sets:
        burst(c, 10)                                            # every instance is loaded and has run
    for _ in range(args.repeats):
        for c in sets:
            ms[c].append(burst(c, args.advances))
    res = {'cells': 2*args.nx*args.ny, 'particles': args.particles, 'advances': args.advances, 'repeats': args.repeats,
           'diffusivity': K, 'dt_move': dt_move}
    for c in sets:
        res['ms_' + c] = {'median': float(np.median(ms[c])), 'min': float(min(ms[c])), 'max': float(max(ms[c]))}
        res['active_' + c] = int((dev.particles_read(sets[c])[2] == 0).sum())
    res['walk_over_old'] = res['ms_walk']['median']/res['ms_old']['median']
    res['plain_over_old'] = res['ms_plain']['median']/res['ms_old']['median']
    print(json.dumps(res))
    dev.close()


if __name__ == '__main__':
    main()
