"""csrc/swe2d_fuse.h, swe_fuse123_kernel after round 22: the staging slot a lane gathers comes from the third plane of its record
(csrc/swe2d_tiles.h: LaneRecords::lane_slot) instead of two per-tile arrays, the staging area has the layout of the state planes
(kStagingPlanes: the lane writes its slot's six values at its own index of six planes of P1, stage 1 reads every trace with the
component step of the tile's own planes), and stages 2 and 3 are two calls of one body.

None of it may change a bit.  The three-stage launch is forced (SWE2D_OPT_FUSED_STAGES = 3, the dataflow kernel off) and asserted
active; the state after 1 and after 3 steps is compared with ``==`` as raw 64-bit patterns (``view(int64)``: the sign of a zero
counts) with the one three stage launches per step leave.  The reference of a mesh is computed once and shared by its tilings.  The
plane and the layout themselves are checked on the host (tests/test_tile_layout.py)."""
import numpy as np
import pytest

import slot_cases

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _run(case, fused, dt=0.5, tile_setup=None, retile=None):
    """[(uv, eta) after 1 step, after 3 steps], tiles at the end.  retile(dev): called after the first step (another tile table on the
    same handle)"""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = case[:4]
    dev = Swe2dDevice(mesh, bath, dt)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
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
    if fused and retile:
        retile(dev)
        on, tiles, _, _ = dev.fused_triple_info()
        assert on, tiles
    dev.advance(2)
    out.append(dev.get_state())
    dev.close()
    return out, tiles


def _reference(case, dt=0.5):
    ref, _ = _run(case, False, dt=dt)
    assert np.isfinite(ref[1][1]).all() and np.abs(ref[0][1] - case[3]).max() > 0.0 and np.abs(ref[1][1] - ref[0][1]).max() > 0.0
    for a in ref:
        for x in a:
            x.setflags(write=False)
    return ref


def _same_bits(ref, case, **kw):
    got, tiles = _run(case, True, **kw)
    for (u0, e0), (u3, e3) in zip(ref, got):
        assert (_bits(u0) == _bits(u3)).all() and (_bits(e0) == _bits(e3)).all()
    return tiles


@pytest.fixture(scope='module')
def rect(hip_lib):
    """33 x 24 quads = 1584 triangles with walls on all sides, its patches of 11 x 8 and of 5 x 3 quads, and the stage launches' states"""
    from thetis_amd import ordering
    case = slot_cases.rectangle(33, 24)
    orders = {p: ordering.triple_tile_order(case[0], *p) for p in ((11, 8), (5, 3))}
    return case, {p: (lambda dev, o=o: dev.fused_set_triple_tiles(*o)) for p, o in orders.items()}, _reference(case)


def test_nine_tiles_all_four_rotations_walls_on_all_sides(rect):
    """3 x 3 patches: tiles 0 .. 8 have the rotations 0, 2, 0, 3, 1, 0, 2, 1, 3; every tile touches a wall and has padding lanes"""
    case, tilings, ref = rect
    assert _same_bits(ref, case, tile_setup=tilings[11, 8]) == 9


def test_fifty_six_small_tiles(rect):
    """patches of 5 x 3 quads: 30 interior cells, most lanes of a tile are rings, few slots per wave"""
    case, tilings, ref = rect
    assert _same_bits(ref, case, tile_setup=tilings[5, 3]) == 7*8


def test_a_table_rebuilt_on_the_same_handle_after_a_step(rect):
    """swe2d_fused_set_triple_tiles a second time, patches of 5 x 3 after the first step: tables, records and the slot plane are built
    and uploaded again, the first ones freed"""
    case, tilings, ref = rect
    assert _same_bits(ref, case, tile_setup=tilings[11, 8], retile=tilings[5, 3]) == 7*8


def test_delaunay_tiles(hip_lib):
    """runs of a coarse Hilbert order on a Delaunay mesh (tests/slot_cases.py): ragged tiles, one of them with 138 staging slots - 35
    lanes of every wave gather one"""
    case = slot_cases.tilings()['delaunay_hilbert']
    mesh = case[0]
    p = mesh.cell_xy()
    per = sum(np.hypot(*(p[:, (i + 1) % 3] - p[:, i]).T) for i in range(3))
    dt = 0.05*float((2*mesh.cell_areas()/per).min())/(np.sqrt(9.81*20.0) + 1.0)       # CFL-limited: small and thin cells
    assert _same_bits(_reference(case, dt), case, dt=dt, tile_setup=case[4]) > 8


def _twelve_cells(n_steps, below_by):
    """slot_cases.rectangle(3, 2): 12 triangles, one tile, every lane's slot word is the sentinel, 244 padding lanes.  A mesh below 64
    cells reaches the three-stage kernel through swe2d_solve_step_cells only (csrc/swe2d_plan.hip), stage 3 on [0, n - below_by).
    Between the steps the cells from cell_end on are set again, as a halo exchange would, the same way on both paths: the fused launch
    leaves there what the other state buffer held, the stage launches U(0)."""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = slot_cases.rectangle(3, 2)
    n = mesh.num_cells
    cell_end = n - below_by

    def run(fused):
        dev = Swe2dDevice(mesh, bath, 0.5)
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3 if fused else 0)
        if fused:
            on, tiles, _, _ = dev.fused_step_info()
            assert on and tiles == 1, (on, tiles)            # the three-stage kernel is what solve_step_cells launches
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
    assert len(below) == n - below_by == 12 - below_by and np.abs(e0[below] - eta[below]).max() > 0.0
    assert (_bits(u0) == _bits(u3)).all() and (_bits(e0) == _bits(e3)).all()


@pytest.mark.parametrize('n_steps', [1, 3])
def test_one_tile_without_a_slot(hip_lib, n_steps):
    _twelve_cells(n_steps, 0)


@pytest.mark.parametrize('n_steps', [1, 3])
def test_solve_step_cells_with_cell_end_below_the_cell_count(hip_lib, n_steps):
    _twelve_cells(n_steps, 3)
