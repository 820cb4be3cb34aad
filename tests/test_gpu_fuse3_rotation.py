"""csrc/swe2d_fuse.h, swe_fuse123_kernel with rotated tiles and stored cell constants (round 10).

A tile's roles [interior | ring 1 | ring 2 | padding] sit on the physical lanes (role + 64*rot) & 255, rot per tile from the tile
number (csrc/swe2d_tiles.h: SWE_FUSE3_ROT); stage 1 leaves the facet lengths, their reciprocals and 1/twoA in LDS and stages 2
and 3 read them back.  Neither may change a bit: the yardstick is the one of tests/test_gpu_parity.py::test_fused_stage_triple... -
the three-stage launch against three stage launches, ``==`` on the float64 arrays after 3 steps, the path switched through
SWE2D_OPT_FUSED_STAGES.

The tile table itself (each cell interior in exactly one tile, neighbour-lane fields pointing at physical lanes, n_inner <= n_mid <=
256) cannot be read back through the ABI of include/swe2d.h: tests/test_tile_tables.py checks it on the host, here it is covered by
the bitwise comparisons - a neighbour field that pointed at the wrong lane, a cell updated twice or not at all, or a count that cut
a ring short would each change the state the launches leave."""
import os

import numpy as np
import pytest

from helpers import channel_case

pytestmark = pytest.mark.gpu

COAST = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh')


def _rot(tile):
    """csrc/swe2d_tiles.h SWE_FUSE3_ROT: the top two bits of tile x 2^32/phi"""
    return ((tile*0x9E3779B1) & 0xffffffff) >> 30


def _three_steps(mesh, bath, uv, eta, dt, fused, setup=None, **kw):
    """state after 3 steps by the three-stage launch (fused) or by stage launches; the number of tiles"""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    dev = Swe2dDevice(mesh, bath, dt, **kw)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
    if setup:
        setup(dev)
    dev.set_state(uv, eta)
    tiles = 0
    if fused:
        on, tiles, ring1, ring2 = dev.fused_triple_info()
        assert on and tiles > 0 and ring1 > 0 and ring2 > 0, (on, tiles, ring1, ring2)
    dev.advance(3)
    out = dev.get_state()
    dev.close()
    return out, tiles


def _same_bits(mesh, bath, uv, eta, dt, setup=None, **kw):
    (u0, e0), _ = _three_steps(mesh, bath, uv, eta, dt, False, setup, **kw)
    (u3, e3), tiles = _three_steps(mesh, bath, uv, eta, dt, True, setup, **kw)
    assert np.isfinite(e0).all() and np.abs(e0 - eta).max() > 0.0
    assert np.array_equal(u0, u3) and np.array_equal(e0, e3)
    return tiles


@pytest.fixture(scope='module')
def small():
    """RectangleMesh(24, 16): 768 triangles, closed walls all round - boundary cells in every wave of the rotated tiles"""
    return channel_case(nx=24, ny=16, lx=100e3, ly=50e3, seed=21, amp_eta=0.3, amp_u=0.2)


@pytest.mark.parametrize('nonlin,lf', [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize('tiling', ['runs', 'patches_6x4'])
def test_rotated_tiles_give_the_bits_of_the_stage_launches(hip_lib, small, tiling, nonlin, lf):
    """'runs': the tiles the library cuts by itself from the device numbering.  Next to closed walls the rings are short, so the 768
    cells make 4 tiles of 180-203 interior cells (rot 0, 2, 0, 3), the last one 248 of 256 lanes.  'patches_6x4': the same mesh cut as
    caller's patches of 6 x 4 quads - 16 tiles, so that every rot occurs, each with many padding lanes wherever rot puts them."""
    from thetis_amd import ordering
    mesh, bath, uv, eta = small
    assert mesh.num_cells == 768

    def setup(dev):
        if tiling == 'patches_6x4':
            dev.fused_set_triple_tiles(*ordering.triple_tile_order(mesh, 6, 4))
    tiles = _same_bits(mesh, bath, uv, eta, 0.5, setup, use_nonlinear_equations=nonlin, use_lax_friedrichs_velocity=lf)
    if tiling == 'runs':
        assert tiles >= 4 and {_rot(t) for t in range(tiles)} >= {0, 2, 3}, tiles
    else:
        assert tiles == 16 and {_rot(t) for t in range(tiles)} == {0, 1, 2, 3}, tiles


def test_rotated_tiles_with_source_terms(hip_lib, small):
    """Coriolis and Manning drag: the instances with source terms (two workgroups per CU), which keep twoA for the drag"""
    from thetis_amd import _lib
    mesh, bath, uv, eta = small
    cxy = mesh.cell_xy()

    def setup(dev):
        dev.set_field(_lib.FIELD_CORIOLIS, 1e-4*(1.0 + cxy[:, :, 1]/50e3))
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    _same_bits(mesh, bath, uv, eta, 0.5, setup)


def test_rotated_tiles_on_an_unstructured_mesh(hip_lib):
    """tests/golden/coast.msh: irregular ring sizes, rings that wrap past lane 255 after the rotation, open and closed boundaries"""
    from thetis_amd.meshio import read_gmsh
    mesh = read_gmsh(COAST)
    x, y = mesh.vertex_xy.T
    bath = 25.0 - 18.0*y/40e3 + 3.0*np.sin(x/9e3)
    rng = np.random.default_rng(5)
    uv = 0.2*rng.normal(size=(mesh.num_cells, 3, 2))
    eta = 0.2*rng.normal(size=(mesh.num_cells, 3))

    def setup(dev):
        dev.set_bc(100, {'elev': 0.3})
        dev.set_bc(300, {'un': 0.0})
    tiles = _same_bits(mesh, bath, uv, eta, 0.2, setup, boundary_len=mesh.boundary_len)
    assert tiles >= 12, tiles


def test_stage_three_skips_cells_beyond_cell_end_on_every_lane(hip_lib, small):
    """A partition's step: swe2d_solve_step_cells(cell_end) with cell_end inside a rotated tile.  Cells below cell_end get the bits of
    the stage launches on the same ranges, cells from cell_end on are not written (the buffer the step lands in keeps what it held)."""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = small
    n = mesh.num_cells
    cell_end = 650                                       # (device numbering) inside the last of the four tiles, rot 3
    marker = 7.25

    def run(fused):
        dev = Swe2dDevice(mesh, bath, 0.5)
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
        if fused:
            on, tiles, _, _ = dev.fused_step_info()
            assert on and tiles >= 4, (on, tiles)
            # what the launch must leave alone: the second state buffer, which becomes the first after the step
            dev.set_state(np.full_like(uv, marker), np.full_like(eta, marker))
            dev.swap_state_buffers()
            dev.set_state(uv, eta)
            dev.solve_step_cells(cell_end)
        else:
            dev.set_state(uv, eta)
            dev.solve_stage_cells(0, 0, n)
            dev.solve_stage_cells(1, 0, n)
            dev.solve_stage_cells(2, 0, cell_end)
        out = dev.get_state()
        perm = None if dev.perm is None else np.asarray(dev.perm)
        dev.close()
        return out, perm

    (u0, e0), perm = run(False)
    (u3, e3), _ = run(True)
    below = np.arange(n)[:cell_end] if perm is None else perm[:cell_end]     # caller's numbers of the device cells [0, cell_end)
    beyond = np.setdiff1d(np.arange(n), below)
    assert np.array_equal(u0[below], u3[below]) and np.array_equal(e0[below], e3[below])
    assert np.abs(e0[below] - eta[below]).max() > 0.0
    assert (u3[beyond] == marker).all() and (e3[beyond] == marker).all()
