#!/usr/bin/env python
"""Where do the ~11 us of a tile's life in the three-stage kernel (csrc/swe2d_fuse.h: swe_fuse123_kernel) go?  Needs a -DSWE_WAVE_TIMING
unity build of the library (THETIS_AMD_LIB): every wave of a sample of workgroups spread evenly over the launch stamps the shader clock
(s_memtime) at 13 points - entry, lane record arrived, the cell's own state arrived, the slot's outside traces arrived, behind each of
the five workgroup barriers, at the end of each stage body, stores drained - and writes them to a debug buffer behind its last store.

    python -c "from thetis_amd import _build; _build.build(unity=True, defines=['SWE_WAVE_TIMING'], lib='variants/wt.so')"
    THETIS_AMD_LIB=variants/wt.so python tools/fuse3_phases.py [--nx 1000 --ny 500]

Per phase: p10, median and p90 in clock ticks and the share of the wave's life (mean phase / mean life), by role class - waves that
run three, two or one stage bodies - and for waves with a slot lane against the others; then the time inside the stage bodies against
the time spent waiting (loads, barriers, stores).  The stamps cost time themselves (about 11 % by the clock's documentation) and each
waits for its own return, which drains the wave's LDS queue: compare SHARES between two builds, not absolute lengths."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, first stamp, last stamp, executing?)  first = None: the latest stamp before `last` that the wave took
PHASES = [('entry -> lane record arrived', 0, 1, False),
          ('record -> own state arrived', 1, 2, False),
          ('own state -> slot traces arrived', 2, 3, False),
          ('LDS stores + barrier 1', None, 4, False),
          ('stage 1 body', 4, 5, True),
          ('barrier 2 (traces of U(0) read)', None, 6, False),
          ('P1 store + barrier 3', 6, 7, False),
          ('stage 2 body', 7, 8, True),
          ('barrier 4 (traces of U(1) read)', None, 9, False),
          ('P1 store + barrier 5', 9, 10, False),
          ('stage 3 body', 10, 11, True),
          ('stores issued and drained', None, 12, False)]


def phase_table(t):
    """t: [waves][13] int64 stamps, 0 = not taken.  Returns ([waves][phases] durations, NaN where the wave has no such phase, life)"""
    n = t.shape[0]
    d = np.full((n, len(PHASES)), np.nan)
    for j, (_, a, b, _) in enumerate(PHASES):
        if a is None:
            prev = np.where(t[:, :b] > 0, t[:, :b], 0).max(axis=1)          # stamps are monotonic: the latest one taken before b
        else:
            prev = t[:, a]
        ok = (t[:, b] > 0) & (prev > 0)
        d[ok, j] = (t[ok, b] - prev[ok]).astype(np.float64)
    return d, (t[:, 12] - t[:, 0]).astype(np.float64)


def report(title, d, life):
    if len(life) == 0:
        print('\n{}: no such wave in the sample'.format(title))
        return
    print('\n{}: {:d} waves, life p10 {:.0f}  median {:.0f}  p90 {:.0f} ticks'.format(title, len(life), *np.percentile(life, [10, 50, 90])))
    print('  {:<36}{:>8}{:>8}{:>8}{:>9}{:>8}'.format('phase', 'p10', 'median', 'p90', 'share %', 'waves'))
    exe = wait = 0.0
    for j, (name, _, _, executing) in enumerate(PHASES):
        x = d[:, j]
        have = ~np.isnan(x)
        if not have.any():
            continue
        share = np.nansum(x)/life.sum()
        exe, wait = exe + share*executing, wait + share*(not executing)
        print('  {:<36}{:8.0f}{:8.0f}{:8.0f}{:9.1f}{:8d}'.format(name, *np.percentile(x[have], [10, 50, 90]), 100.0*share, int(have.sum())))
    print('  inside the stage bodies {:.1f} %   waiting (loads, barriers, stores) {:.1f} %   unaccounted {:.1f} %'.format(
        100.0*exe, 100.0*wait, 100.0*(1.0 - exe - wait)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=1000)
    ap.add_argument('--ny', type=int, default=500)
    ap.add_argument('--steps', type=int, default=20)
    args = ap.parse_args()
    import bench
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = bench.build_case(args.nx, args.ny)
    dev = Swe2dDevice(mesh, bath, bench.DT)
    dev.set_state(uv, eta)
    on, tiles, ring1, ring2 = dev.fused_triple_info()
    if not on:
        raise SystemExit('the three-stage kernel does not take this mesh by itself')
    dev.advance(args.steps)                                  # the stamps are those of the last launch
    dev.synchronize()
    fn = dev.lib.swe2d_debug_read_fuse3_phases
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    info = np.zeros(3, dtype=np.int32)
    dev._ck(fn(dev.h, None, 0, info.ctypes.data))
    words, stamps, max_wg = (int(x) for x in info)
    grid = (tiles + 7)//8*8
    every = (grid + max_wg - 1)//max_wg
    n_wg = (grid + every - 1)//every
    raw = np.zeros((n_wg, 4, words), dtype=np.uint64)
    dev._ck(fn(dev.h, raw.ctypes.data, n_wg, info.ctypes.data))
    dev.close()
    rec = raw.reshape(-1, words)
    ok = ((rec[:, 14] >> np.uint64(44)) & np.uint64(1)) == 1               # (the padding workgroups of the grid return at once)
    rec = rec[ok]
    t = rec[:, :stamps].astype(np.int64)
    bodies = ((rec[:, 14] >> np.uint64(40)) & np.uint64(0xf)).astype(np.int64)
    slot = t[:, 3] > 0
    d, life = phase_table(t)
    print('# tools/fuse3_phases.py: mesh {:d} x {:d}, {:d} triangles, {:d} tiles (ring 1 {:d}, ring 2 {:d} cells); every {:d}. workgroup sampled, {:d} waves'.format(
        args.nx, args.ny, mesh.num_cells, tiles, ring1, ring2, every, len(life)))
    print('# ticks of s_memtime (the shader clock).  The stamps cost time themselves (about 11 % by the clock\'s documentation) and each drains')
    print('# the wave\'s LDS queue: compare the SHARES of two builds, not the lengths.  A body\'s time includes what its wave waits for the')
    print('# SIMD it shares with two other workgroups\' waves and for its LDS reads.')
    report('all waves', d, life)
    for b in (3, 2, 1):
        report('waves that run {:d} stage bod{}'.format(b, 'y' if b == 1 else 'ies'), d[bodies == b], life[bodies == b])
    report('waves with a slot lane', d[slot], life[slot])
    report('waves without a slot lane', d[~slot], life[~slot])
    # the premise of the slot plane: do the outside traces arrive later than the cell's own state?
    arr_own, arr_slot = (t[:, 2] - t[:, 0])[t[:, 2] > 0], (t[:, 3] - t[:, 0])[slot]
    print('\narrival after entry, ticks (p10 median p90): own state {:.0f} {:.0f} {:.0f}'.format(*np.percentile(arr_own, [10, 50, 90]))
          + ('   slot traces {:.0f} {:.0f} {:.0f}'.format(*np.percentile(arr_slot, [10, 50, 90])) if slot.any() else '   (no wave with a slot lane)'))
    both = slot & (t[:, 2] > 0)
    if both.any():
        lag = (t[both, 3] - t[both, 2]).astype(np.float64)
        trip = (t[both, 2] - t[both, 1]).astype(np.float64)
        print('slot traces behind own state in the same wave: p10 {:.0f}  median {:.0f}  p90 {:.0f} ticks   (one trip, record -> own state: median {:.0f})'.format(
            *np.percentile(lag, [10, 50, 90]), np.median(trip)))


if __name__ == '__main__':
    main()
