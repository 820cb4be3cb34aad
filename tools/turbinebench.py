#!/usr/bin/env python
"""What the tidal turbine term costs where it is on, and what a run with source terms but without farms pays for the farm code in
its kernels (reported, not gated).  1 M triangles, flat bed, closed walls, quadratic bottom drag:

    drag only | + a constant-thrust farm on ~10 % of the cells | + a tabulated farm with the upwind correction on the same cells

each timed with HIP events over ``--steps`` steps after a warm-up (swe2d_advance_timed), repeated ``--repeat`` times; and the power
kernel's time per appended row.  ``--drag-only``: the first case alone - what a library without the turbine calls can run
(THETIS_AMD_LIB=<library of the parent commit> for the A/B of the drag-only case).

    python tools/turbinebench.py [--nx 1000 --ny 500 --steps 100 --repeat 5] [--drag-only]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=1000)
    ap.add_argument('--ny', type=int, default=500)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--drag-only', action='store_true')
    args = ap.parse_args()
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    from thetis_amd.mesh import RectangleMesh
    lx, ly = 100e3, 50e3
    mesh = RectangleMesh(args.nx, args.ny, lx, ly)
    n, k = mesh.num_cells, 3
    cxy = mesh.cell_xy()
    x, y = cxy[:, :, 0], cxy[:, :, 1]
    eta = 0.5*np.exp(-((x - 0.5*lx)**2 + (y - 0.5*ly)**2)/(5e3)**2)
    uv = np.stack([1.5 + 0.5*np.sin(x/6130.0 + y/3890.0), 0.5*np.cos(x/4570.0 - y/8230.0)], axis=-1)
    xc = x.mean(axis=1)
    inside = (xc > 0.45*lx) & (xc < 0.55*lx)                     # ~10 % of the cells
    dens = np.where(inside[:, None], 2e-5, 0.0)*np.ones((n, k))

    def farm(kind):
        p = _lib.TurbineParams()
        p.rotor_area, p.projected_diameter, p.rho0 = np.pi*81.0, 18.0, 1000.0
        if kind == 'constant':
            p.thrust_area_const, p.power_const = 0.8*np.pi*81.0, 0.58
        else:
            p.upwind_correction, p.n_table = 1, 5
            for j, (s, c) in enumerate(zip([0.9, 1., 3., 5., 5.001], [0.01, 0.7, 0.7, 0.1, 0.0001])):
                p.speeds[j], p.thrust[j], p.power[j] = s, c, 0.5*c*(1 + (1 - c)**0.5)
        return p

    for case in (['drag only'] if args.drag_only else ['drag only', 'constant farm', 'table + upwind farm']):
        dev = Swe2dDevice(mesh, np.full(mesh.num_vertices, 30.0), 0.25)
        dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, 0.0025)
        if case != 'drag only':
            dev.turbine_farm_set(0, farm('constant' if case.startswith('constant') else 'table'), dens)
        dev.set_state(uv, eta)
        dev.snapshot()
        dev.advance(20)
        ms = []
        for _ in range(args.repeat):
            dev.restore()
            ms.append(dev.advance_timed(args.steps)[0]/args.steps)
        how = 'fused pair' if dev.fused_pair_info()[0] else ('three-stage kernel' if dev.fused_triple_info()[0] else 'stage launches')
        print('{:22s} {:d} cells ({:d} in the farm)  ms/step  min {:.5f}  median {:.5f}  max {:.5f}   [{:}]'.format(
            case, n, int(inside.sum()) if case != 'drag only' else 0, min(ms), float(np.median(ms)), max(ms), how), flush=True)
        if case != 'drag only':
            rows = 200
            dev.turbine_rows_reserve(rows)
            dev.synchronize()
            t0 = time.perf_counter()
            for _ in range(rows):
                dev.turbine_rows_append()
            dev.synchronize()
            dt = (time.perf_counter() - t0)/rows
            out = dev.turbine_rows_read()
            print('{:22s} power row: {:.2f} us per appended row ({:d} rows back to back, host clock), P = {:.6e} W'.format(
                '', 1e6*dt, rows, out[-1, 0]), flush=True)
        dev.close()


if __name__ == '__main__':
    main()
