"""csrc/swe2d_fuse.h, swe_fuse123_kernel: the prologue from the lane records the host decodes once per table (csrc/swe2d_tiles.h:
build_lane_records) - the cell, the three trace words, the vertex byte offsets, bmarkers, per staging slot the two byte offsets.

None of it may change a bit.  The three-stage launch is forced (SWE2D_OPT_FUSED_STAGES = 3, the dataflow kernel off) and asserted
active; the state after 1 and after 3 steps is compared with ``==`` as raw 64-bit patterns (``view(int64)``: the sign of a zero
counts) with the one three stage launches per step leave.  The records themselves are checked on the host (tests/test_tile_records.py)."""
import numpy as np
import pytest

import slot_cases

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(case, fused, dt=0.5, options=None, between=None, tile_setup=None, retile=None, **kw):
    """[(uv, eta) after 1 step, after 3 steps], tiles at the end.  between(dev): called after the first step on both paths;
    retile(dev): called after the first step on the fused path only (another tile table on the same handle)"""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = case[:4]
    dev = Swe2dDevice(mesh, bath, dt, **kw)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
    if options:
        options(dev)
    if fused and tile_setup:
        tile_setup(dev)
    dev.set_state(uv, eta)
    tiles = 0
    if fused:
        on, tiles, _, _ = dev.fused_triple_info()
        assert on and tiles > 0, (on, tiles)                # the three-stage kernel is what the step launches
    out = []
    dev.advance(1)
    out.append(dev.get_state())
    if between:
        between(dev)
    if fused and retile:
        retile(dev)
        on, tiles, _, _ = dev.fused_triple_info()
        assert on, tiles
    dev.advance(2)
    out.append(dev.get_state())
    dev.close()
    return out, tiles


def _same_bits(case, **kw):
    ref, _ = _run(case, False, **{k: v for k, v in kw.items() if k not in ('tile_setup', 'retile')})
    got, tiles = _run(case, True, **kw)
    assert np.isfinite(ref[1][1]).all() and np.abs(ref[0][1] - case[3]).max() > 0.0 and np.abs(ref[1][1] - ref[0][1]).max() > 0.0
    for (u0, e0), (u3, e3) in zip(ref, got):
        assert (_bits(u0) == _bits(u3)).all() and (_bits(e0) == _bits(e3)).all()
    return tiles


@pytest.fixture(scope='module')
def rect():
    """33 x 24 quads = 1584 triangles with walls on all sides, and its patches of 11 x 8 and of 5 x 3 quads"""
    from thetis_amd import ordering
    case = slot_cases.rectangle(33, 24)
    orders = {p: ordering.triple_tile_order(case[0], *p) for p in ((11, 8), (5, 3))}
    return case, {p: (lambda dev, o=o: dev.fused_set_triple_tiles(*o)) for p, o in orders.items()}


def test_nine_tiles_all_four_rotations_walls_on_all_sides(hip_lib, rect):
    """3 x 3 patches: tiles 0 .. 8 have the rotations 0, 2, 0, 3, 1, 0, 2, 1, 3; every tile touches a wall"""
    case, tilings = rect
    assert _same_bits(case, tile_setup=tilings[11, 8]) == 9


def test_delaunay_tiles(hip_lib):
    """runs of a coarse Hilbert order on a Delaunay mesh (tests/slot_cases.py): ragged tiles, one of them with 138 staging slots"""
    case = slot_cases.tilings()['delaunay_hilbert']
    mesh = case[0]
    p = mesh.cell_xy()
    per = sum(np.hypot(*(p[:, (i + 1) % 3] - p[:, i]).T) for i in range(3))
    dt = 0.05*float((2*mesh.cell_areas()/per).min())/(np.sqrt(9.81*20.0) + 1.0)       # CFL-limited: small and thin cells
    assert _same_bits(case, dt=dt, tile_setup=case[4]) > 8


@pytest.mark.parametrize('n_steps', [1, 3])
def test_twelve_cells_through_solve_step_cells_with_cell_end_below_the_cell_count(hip_lib, n_steps):
    """one tile, no staging slot, 244 padding lanes.  Between the steps the cells from cell_end on are set again, as a halo exchange
    would, the same way on both paths: the fused launch leaves there what the other state buffer held, the stage launches U(0)."""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = slot_cases.rectangle(3, 2)
    n = mesh.num_cells
    cell_end = n - 3

    def run(fused):
        dev = Swe2dDevice(mesh, bath, 0.5)
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
        if fused:
            on, tiles, _, _ = dev.fused_step_info()
            assert on and tiles == 1, (on, tiles)
        perm = np.arange(n) if dev.perm is None else np.asarray(dev.perm)
        below = perm[:cell_end]
        u, e = uv.copy(), eta.copy()
        for _ in range(n_steps):
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
    assert len(below) == 9 and np.abs(e0[below] - eta[below]).max() > 0.0
    assert (_bits(u0) == _bits(u3)).all() and (_bits(e0) == _bits(e3)).all()


def test_a_boundary_kind_changed_between_two_steps_under_the_same_table(hip_lib, rect):
    """marker 1 is an open boundary with an elevation in step 1 and with a normal velocity in steps 2 and 3: swe2d_set_bc changes the
    marker's kind, the table is not rebuilt - bkind1 is a look-up in the kernel, not a field of the lane record"""
    case, tilings = rect

    def options(dev):
        dev.set_bc(1, {'elev': 0.2})
        dev.set_bc(3, {'un': 0.01})

    def between(dev):
        dev.set_bc(1, {'un': -0.02})

    assert _same_bits(case, options=options, between=between, tile_setup=tilings[11, 8]) == 9


def test_source_terms(hip_lib, rect):
    """Coriolis and Manning drag: an instance with two workgroups per compute unit"""
    from thetis_amd import _lib
    case, tilings = rect
    cxy = case[0].cell_xy()

    def options(dev):
        dev.set_field(_lib.FIELD_CORIOLIS, 1e-4*(1.0 + cxy[:, :, 1]/60e3))
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    assert _same_bits(case, options=options, tile_setup=tilings[11, 8]) == 9


def test_other_patches_on_the_same_handle(hip_lib, rect):
    """swe2d_fused_set_triple_tiles a second time, patches of 5 x 3 after the first step: tables and records are built again"""
    case, tilings = rect
    assert _same_bits(case, tile_setup=tilings[11, 8], retile=tilings[5, 3]) == 7*8
