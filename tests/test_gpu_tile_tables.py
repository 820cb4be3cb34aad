"""The tile tables of the fused stage kernels in the compiled library (csrc/swe2d_api_fuse.hip: one TileSet per kernel, upload_tiles,
free_tiles): built, freed and built again on one handle as the order changes.

What swe2d_fused_pair_info / swe2d_fused_triple_info report after each change must be the entry of tests/golden/tile_tables.json for
that order - the tables tests/test_tile_tables.py checks cell by cell on the host are the ones the library builds - and two SSPRK33
steps by the fused kernels must leave the bits of the stage launches (``==`` on the float64 arrays), whatever was built before."""
import json
import os

import numpy as np
import pytest

import tile_cases
from helpers import channel_case, quad_case

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tile_tables.json')))


def _expected(key):
    g = GOLDEN[key]
    return (True, g['n_tiles'], g['ring'][0], g['ring'][1])


def _device(mesh, bath, dt=0.5):
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    dev = Swe2dDevice(mesh, bath, dt)
    dev.set_option(_lib.OPT_FLOW, 0)                        # (768 cells: swe2d_advance would take the dataflow kernel)
    return dev


def _two_steps(dev, mode, uv, eta):
    from thetis_amd import _lib
    dev.set_option(_lib.OPT_FUSED_STAGES, mode)             # 0 stage launches | 1 the stage pair | 3 all three stages in one launch
    dev.set_state(uv, eta)
    dev.advance(2)
    return dev.get_state()


def _check(dev, kinds, case, uv, eta, ref):
    """the counts of ``case`` and the bits of the stage launches, by every fused kernel of the handle"""
    from thetis_amd import _lib
    counts = []
    for kind in kinds:
        dev.set_option(_lib.OPT_FUSED_STAGES, 3 if kind == 'triple' else 1)
        info = dev.fused_triple_info() if kind == 'triple' else dev.fused_pair_info()[:3] + (0,)
        assert info == _expected(case + ':' + kind), (case, kind, info)
        counts.append(info)
        u, e = _two_steps(dev, 3 if kind == 'triple' else 1, uv, eta)
        assert np.array_equal(u, ref[0]) and np.array_equal(e, ref[1]), (case, kind)
    return counts


@pytest.mark.parametrize('cells', ['triangles', 'quadrilaterals'])
def test_tables_are_rebuilt_when_the_order_changes(hip_lib, cells):
    tri = cells == 'triangles'
    name = 'tri24x16' if tri else 'quad25x16'
    kinds = ('pair', 'triple') if tri else ('quad',)
    mesh, bath, uv, eta = (channel_case(nx=24, ny=16, lx=100e3, ly=50e3, seed=21, amp_eta=0.3, amp_u=0.2) if tri else
                           quad_case(nx=25, ny=16, lx=100e3, ly=50e3, seed=22, amp_eta=0.3, amp_u=0.2))
    case = tile_cases.cases()[name]
    assert np.array_equal(np.asarray(mesh.cells), np.asarray(case['mesh'].cells))
    stages = _device(mesh, bath)
    ref = _two_steps(stages, 0, uv, eta)
    stages.close()
    assert np.isfinite(ref[1]).all() and np.abs(ref[1] - eta).max() > 0.0

    dev = _device(mesh, bath)
    assert np.array_equal(dev.perm, tile_cases.device_numbering(mesh)[0])        # the golden cases are in this numbering
    first = _check(dev, kinds, name, uv, eta, ref)                              # 1. the device numbering
    dev.fused_set_order(tile_cases.hilbert_order(mesh))
    second = _check(dev, kinds, name + '_hilbert', uv, eta, ref)                # 2. another order: freed and built again
    assert second != first
    dev.fused_set_order(None)
    assert _check(dev, kinds, name, uv, eta, ref) == first                      # 3. back

    if tri:                                                 # the two-ring tiles' own order and starts, then without
        from thetis_amd import ordering
        dev.fused_set_triple_tiles(*ordering.triple_tile_order(mesh, 6, 4))
        _check(dev, ('triple',), name + '_patches6x4', uv, eta, ref)
        _check(dev, ('pair',), name, uv, eta, ref)          # (the pair's tables are not the patches')
        dev.fused_set_triple_tiles(None)                    # n_starts = 0: the pair's order again
        assert _check(dev, ('triple',), name, uv, eta, ref) == first[1:]
    dev.close()
