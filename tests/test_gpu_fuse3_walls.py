"""csrc/swe2d_fuse.h, swe_fuse123_kernel with the wall cells of a tile on consecutive roles (csrc/swe2d_tiles.h: TileSpec::group_walls)
and the zeroing of a boundary facet's flux behind a wave-uniform branch (csrc/swe2d_tri.h: swe_tri_facet<.., WAVEB>).

Neither may change a bit.  The three-stage launch is forced (SWE2D_OPT_FUSED_STAGES = 3, the dataflow kernel off) and asserted active;
the state after 1 and after 3 steps is compared with ``==`` as raw 64-bit patterns with the one three stage launches per step leave.

Meshes: 23 x 17 quads in patches of 11 x 8 (nine tiles: corner, edge and ragged patches, the rotations 0, 2, 0, 3, 1, 0, 2, 1, 3) and
34 x 25 quads (sixteen tiles, four of them without a wall cell in their interior), each with closed walls all round and with marker 1
an open boundary with an elevation - a second ``kind`` in the boundary pass - and one patch by itself, 11 x 8 quads: every cell of the
perimeter is a wall cell, the corner cells with two wall facets run the boundary pass twice, and waves with and without a wall cell sit
in one workgroup - the smallest shape on which the wave-uniform test and the two-pass corner case can both go wrong.  (A tile's
rotation follows from its number, so the single tile has rotation 0.)  The tables themselves: tests/test_tile_walls.py, on the host."""
import numpy as np
import pytest

import slot_cases

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(case, fused, patches, open_marker):
    """[(uv, eta) after 1 step, after 3 steps], tiles"""
    from thetis_amd import _lib, ordering
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = case[:4]
    dev = Swe2dDevice(mesh, bath, 0.5)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
    if open_marker:
        dev.set_bc(1, {'elev': 0.2})
    tiles = 0
    if fused:
        dev.fused_set_triple_tiles(*ordering.triple_tile_order(mesh, *patches))
    dev.set_state(uv, eta)
    if fused:
        on, tiles, _, _ = dev.fused_triple_info()
        assert on and tiles > 0, (on, tiles)
    out = []
    dev.advance(1)
    out.append(dev.get_state())
    dev.advance(2)
    out.append(dev.get_state())
    dev.close()
    return out, tiles


_REF = {}


def _same_bits(shape, open_marker):
    case = slot_cases.rectangle(*shape)
    key = (shape, open_marker)
    if key not in _REF:
        _REF[key] = _run(case, False, (11, 8), open_marker)[0]
    ref = _REF[key]
    got, tiles = _run(case, True, (11, 8), open_marker)
    assert np.isfinite(ref[1][1]).all() and np.abs(ref[0][1] - case[3]).max() > 0.0 and np.abs(ref[1][1] - ref[0][1]).max() > 0.0
    for (u0, e0), (u3, e3) in zip(ref, got):
        assert (_bits(u0) == _bits(u3)).all() and (_bits(e0) == _bits(e3)).all()
    return tiles


@pytest.mark.parametrize('open_marker', [False, True], ids=['walls', 'open_side'])
@pytest.mark.parametrize('shape,tiles', [((23, 17), 9), ((34, 25), 16), ((11, 8), 1)], ids=['23x17', '34x25', 'one_patch'])
def test_grouped_wall_cells_give_the_bits_of_the_stage_launches(hip_lib, shape, tiles, open_marker):
    assert _same_bits(shape, open_marker) == tiles
