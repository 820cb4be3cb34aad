#!/usr/bin/env python
"""Where do the waves of the three-stage kernel (csrc/swe2d_fuse.h: swe_fuse123_kernel) run, and how is its work spread over the four
SIMDs of a compute unit?  Needs a -DSWE_WAVE_TIMING unity build of the library (THETIS_AMD_LIB): every wave of the launch records
HW_ID, XCC_ID and the number of stage bodies it executed (1 to 3).

    python -c "from thetis_amd import _build; _build.build(unity=True, defines=['SWE_WAVE_TIMING'], lib='variants/wt.so')"
    THETIS_AMD_LIB=variants/wt.so python tools/fuse3timing.py [--nx 1000 --ny 500]

(add "'SWE_FUSE3_ROT(tile)=0'" to the defines for the layout without rotation: the short wave is then wave 3 of every workgroup)"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WT_MAX = 8192               # csrc/swe2d_kernels.h SWE_WT_MAX


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
    dev.advance(args.steps)                                  # the records are those of the last launch
    dev.synchronize()
    fn = dev.lib.swe2d_debug_read_wave_timing
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    ts = np.zeros(6*WT_MAX, dtype=np.uint64)
    dev._ck(fn(dev.h, ts.ctypes.data))
    dev.close()
    grid = (tiles + 7)//8*8
    nw = min(4*grid, 6*WT_MAX)
    rec = ts[:nw]
    ok = ((rec >> np.uint64(44)) & np.uint64(1)) == 1
    wave = np.arange(nw) & 3
    hw = rec & np.uint64(0xffffffff)
    # gfx9 HW_ID: wave_id [3:0], simd_id [5:4], pipe [7:6], cu_id [11:8], sh_id [12], se_id [15:13]; XCC_ID in bits 32..35 of the record
    simd = ((hw >> np.uint64(4)) & np.uint64(3)).astype(np.int64)
    cu = (((hw >> np.uint64(8)) & np.uint64(0xff)) | (((rec >> np.uint64(32)) & np.uint64(0xf)) << np.uint64(8))).astype(np.int64)
    bodies = ((rec >> np.uint64(40)) & np.uint64(0xf)).astype(np.int64)
    simd, cu, bodies, wave = simd[ok], cu[ok], bodies[ok], wave[ok]
    print('mesh {:d} x {:d}: {:d} triangles, {:d} tiles (ring 1 {:d}, ring 2 {:d} cells), {:d} of {:d} waves recorded'.format(
        args.nx, args.ny, mesh.num_cells, tiles, ring1, ring2, int(ok.sum()), 4*tiles))
    print('\nwave of the workgroup -> SIMD it ran on (waves)')
    print('        ' + ''.join('  simd {:d}'.format(s) for s in range(4)) + '   stage bodies per wave (mean)')
    for w in range(4):
        row = [int(((wave == w) & (simd == s)).sum()) for s in range(4)]
        print('wave {:d}  '.format(w) + ''.join('{:8d}'.format(r) for r in row) + '   {:.3f}'.format(bodies[wave == w].mean()))
    print('\nSIMD of wave w, relative to the SIMD of wave 0 of the same workgroup: (simd_w - simd_0) & 3')
    for w in range(1, 4):                                    # (a workgroup records all four waves or none)
        d = (simd[wave == w] - simd[wave == 0]) & 3
        print('wave {:d}  '.format(w) + ''.join('{:8d}'.format(int((d == k).sum())) for k in range(4)))
    print('\nstage bodies executed per SIMD, summed over the launch')
    tot = np.array([bodies[simd == s].sum() for s in range(4)], dtype=np.float64)
    print('        ' + ''.join('{:8d}'.format(int(t)) for t in tot) + '   max/mean {:.4f}'.format(tot.max()/tot.mean()))
    # per compute unit: the busiest SIMD sets the time the unit needs
    cus = np.unique(cu)
    per = np.zeros((len(cus), 4))
    idx = np.searchsorted(cus, cu)
    np.add.at(per, (idx, simd), bodies)
    ratio = per.max(axis=1)/per.mean(axis=1)
    print('\nper compute unit ({:d} units): stage bodies on the busiest SIMD / mean of its four SIMDs'.format(len(cus)))
    print('  mean {:.4f}  median {:.4f}  p90 {:.4f}  max {:.4f}   (1.0000 = even; 12/11 = 1.0909 when one SIMD hosts every short wave)'.format(
        ratio.mean(), np.median(ratio), np.percentile(ratio, 90), ratio.max()))
    print('  spread (max - min)/mean per unit: mean {:.4f}  max {:.4f}'.format(
        ((per.max(axis=1) - per.min(axis=1))/per.mean(axis=1)).mean(), ((per.max(axis=1) - per.min(axis=1))/per.mean(axis=1)).max()))
    print('  stage bodies per unit: mean {:.1f}  min {:.0f}  max {:.0f}'.format(per.sum(axis=1).mean(), per.sum(axis=1).min(), per.sum(axis=1).max()))


if __name__ == '__main__':
    main()
