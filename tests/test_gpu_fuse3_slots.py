"""csrc/swe2d_fuse.h, swe_fuse123_kernel: the traces from outside a tile gathered by staging slot (lane 64*(s & 3) + (s >> 2) loads the
six values of slot s, csrc/swe2d_tiles.h: slot_src), trace addresses held in bytes, stages 2 and 3 with every trace inside the tile.

None of it may change a bit.  The three-stage launch is forced (SWE2D_OPT_FUSED_STAGES = 3, the dataflow kernel off) and asserted
active; 2-3 steps; the state compared as raw 64-bit patterns (``view(int64)``: the sign of a zero counts) with the one three stage
launches per step leave.  The tables themselves are checked on the host (tests/test_tile_slots.py, same meshes)."""
import numpy as np
import pytest

import slot_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def tilings():
    return slot_cases.tilings()


def _steps(case, fused, n_steps=3, options=None, step_cells=False, **kw):
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta, tile_setup = case
    dev = Swe2dDevice(mesh, bath, kw.pop('dt', 0.5), **kw)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
    if options:
        options(dev)
    if fused and tile_setup:
        tile_setup(dev)
    dev.set_state(uv, eta)
    tiles = 0
    if fused:
        on, tiles, _, _ = dev.fused_step_info() if step_cells else dev.fused_triple_info()
        assert on and tiles > 0, (on, tiles)                # the three-stage kernel is what the step launches
    if fused and step_cells:
        for _ in range(n_steps):
            dev.solve_step_cells(mesh.num_cells)
    else:
        dev.advance(n_steps)
    out = dev.get_state()
    dev.close()
    return out, tiles


def _same_bits(case, **kw):
    (u0, e0), _ = _steps(case, False, **kw)
    (u3, e3), tiles = _steps(case, True, **kw)
    assert np.isfinite(e0).all() and np.abs(e0 - case[3]).max() > 0.0
    assert np.array_equal(np.ascontiguousarray(u0).view(np.int64), np.ascontiguousarray(u3).view(np.int64))
    assert np.array_equal(np.ascontiguousarray(e0).view(np.int64), np.ascontiguousarray(e3).view(np.int64))
    return tiles


def test_one_tile_without_staging_slots(hip_lib, tilings):
    """3 x 2 quads = 12 triangles: the tile holds the whole mesh, n_slots = 0, no lane gathers.  (swe2d_advance keeps its stage launches
    below 64 cells even when the option forces the kernel: the step is launched as a partition launches it, swe2d_solve_step_cells on
    all cells.)"""
    assert _same_bits(tilings['tri3x2'], step_cells=True) == 1


@pytest.mark.parametrize('patches', ['11x8', '5x3'])
def test_ragged_last_tiles(hip_lib, tilings, patches):
    """23 x 17 quads cut into patches of 11 x 8 (3 x 3 tiles, the last row 1 quad high, the last column 1 wide) and of 5 x 3 (30 tiles)"""
    tiles = _same_bits(tilings['tri23x17_patches' + patches])
    assert tiles == (9 if patches == '11x8' else 30)


def test_open_boundaries_on_two_sides(hip_lib, tilings):
    """markers 1 and 3 meet in a corner: cells with two boundary facets, each with a boundary condition of its own"""
    def options(dev):
        dev.set_bc(1, {'elev': 0.2})
        dev.set_bc(3, {'un': 0.01})
    _same_bits(tilings['tri23x17_patches11x8'], options=options)


def test_linear_equations_without_lax_friedrichs(hip_lib, tilings):
    _same_bits(tilings['tri23x17_patches11x8'], use_nonlinear_equations=False, use_lax_friedrichs_velocity=False)


def test_source_terms(hip_lib, tilings):
    """Coriolis and Manning drag: the instances with two workgroups per compute unit"""
    from thetis_amd import _lib
    cxy = tilings['tri23x17_patches11x8'][0].cell_xy()

    def options(dev):
        dev.set_field(_lib.FIELD_CORIOLIS, 1e-4*(1.0 + cxy[:, :, 1]/60e3))
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    _same_bits(tilings['tri23x17_patches11x8'], options=options)


def test_delaunay_tiles_with_more_than_128_slots(hip_lib, tilings):
    """runs of a coarse Hilbert order on a Delaunay mesh: a tile with 138 staging slots (tests/test_tile_slots.py), so that the
    lanes 32 and up of every wave gather too"""
    mesh = tilings['delaunay_hilbert'][0]
    # CFL-limited step: Delaunay meshes contain small and thin cells (inradius ~ 2A/perimeter)
    p = mesh.cell_xy()
    per = sum(np.hypot(*(p[:, (i + 1) % 3] - p[:, i]).T) for i in range(3))
    dt = 0.05*float((2*mesh.cell_areas()/per).min())/(np.sqrt(9.81*20.0) + 1.0)
    tiles = _same_bits(tilings['delaunay_hilbert'], dt=dt, n_steps=2)
    assert tiles > 8, tiles


def test_cell_end_below_the_cell_count(hip_lib, tilings):
    """swe2d_solve_step_cells(cell_end), two steps.  Between the steps the cells from cell_end on are set again, as a halo exchange
    would, the same way on both paths: the fused launch leaves there what the other state buffer held, the stage launches U(0)."""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta, tile_setup = tilings['tri23x17_patches11x8']
    n = mesh.num_cells
    cell_end = n - 150

    def run(fused):
        dev = Swe2dDevice(mesh, bath, 0.5)
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
        if fused:
            tile_setup(dev)
            on, tiles, _, _ = dev.fused_step_info()
            assert on and tiles == 9, (on, tiles)
        perm = np.arange(n) if dev.perm is None else np.asarray(dev.perm)
        below = perm[:cell_end]
        u, e = uv.copy(), eta.copy()
        for _ in range(2):
            dev.set_state(u, e)
            if fused:
                dev.solve_step_cells(cell_end)
            else:
                dev.solve_stage_cells(0, 0, n)
                dev.solve_stage_cells(1, 0, n)
                dev.solve_stage_cells(2, 0, cell_end)
            u1, e1 = dev.get_state()
            u, e = uv.copy(), eta.copy()
            u[below], e[below] = u1[below], e1[below]
        dev.close()
        return u, e, below

    u0, e0, below = run(False)
    u3, e3, _ = run(True)
    assert np.abs(e0[below] - eta[below]).max() > 0.0
    assert np.array_equal(u0.view(np.int64), u3.view(np.int64)) and np.array_equal(e0.view(np.int64), e3.view(np.int64))
