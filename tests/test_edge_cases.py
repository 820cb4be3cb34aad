"""CPU: what tests/test_gpu_launch_edges.py runs on - the size lists, the configurations and the range drivers of tests/edge_cases.py - checked
with the references alone.  The sizes meet the edges they are there for (counted, so that an edit cannot thin the lists silently), the
numpy oracle is finite on every mesh and configuration, the wetting-drying meshes really are partly dry, and the range drivers, run on
the C restatement (tests/cpu_device.py, for what it covers: constants, no wetting-drying, no viscosity), meet the conditions the GPU
file asks of the HIP library: ranges give the bits of the whole launch, cells outside a range keep theirs."""
import numpy as np
import pytest

import edge_cases as ec
from cpu_device import CpuSwe2dDevice


def _counts(kind):
    return [ec.num_cells(kind, nx, ny) for nx, ny in ec.sizes(kind)]


def test_size_lists_sit_on_the_edges_of_waves_workgroups_and_tiles():
    tri, quad = _counts('tri'), _counts('skew')
    assert tri == [2, 6, 62, 64, 66, 126, 128, 130, 190, 192, 194, 254, 256, 258, 510, 512, 514]
    assert quad == [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
    assert _counts('warp') == quad and max(tri + quad) == 514
    # a wave / stage workgroup of 64 cells
    assert {n % 64 for n in quad} >= {0, 1, 63} and {n % 64 for n in tri} >= {0, 2, 62}
    # a helper workgroup or a tile of 256 lanes, a tile's 192 interior cells
    assert {n % 256 for n in quad} >= {0, 1, 255} and {n % 256 for n in tri} >= {0, 2, 254}
    assert {191, 192, 193} <= set(quad) and {190, 192, 194} <= set(tri)
    for m in (64, 128, 192, 256):
        assert {m - 1, m, m + 1} <= set(quad) and {m - 2, m, m + 2} <= set(tri), m
    assert {510, 512, 514} <= set(tri)
    # below one wave, the one-cell mesh, strips one cell wide (every cell with two or three boundary facets of different markers)
    assert 1 in quad and 2 in tri and sum(n < 64 for n in quad) == 3 and sum(n < 64 for n in tri) == 3
    assert sum(ny == 1 for _, ny in ec.TRI_SIZES) == 6 and sum(ny == 1 for _, ny in ec.QUAD_SIZES) == 6
    assert len(ec.TRI_SIZES) == 17 and len(ec.QUAD_SIZES) == 14
    # configurations a, b, c on every size, d up to 258 / 257 cells: 17*3 + 14 triangle cases, (14*3 + 14) per quadrilateral geometry
    cases = ec.size_cases()
    assert len(cases) == len(set(cases)) == 65 + 2*56 and len(ec.tracer_cases()) == 17 + 2*14
    assert sum(c[3] == 'd' for c in cases) == 14 + 2*14
    assert all(ec.num_cells(*c[:3]) <= ec.VISC_MAX_CELLS for c in cases if c[3] == 'd')
    assert {c[3] for c in cases if ec.num_cells(*c[:3]) > ec.VISC_MAX_CELLS} == {'a', 'b', 'c'}


def test_strips_have_cells_with_boundary_facets_of_different_markers():
    for kind, nx in (('tri', 31), ('skew', 127), ('warp', 257)):
        nbr = np.asarray(ec.mesh_case(kind, nx, 1)[0].cell_nbr)
        per_cell = [set(-row[row < 0]) for row in nbr]
        assert all(len(m) >= (1 if kind == 'tri' else 2) for m in per_cell)
        assert max(len(m) for m in per_cell) >= (2 if kind == 'tri' else 3)
        assert set().union(*per_cell) == {1, 2, 3, 4}


def test_split_points_and_ranges():
    assert ec.split_points(130) == [0, 1, 63, 64, 65, 127, 129, 130]
    assert ec.split_points(514) == [0, 1, 63, 64, 65, 127, 129, 513, 514]
    with pytest.raises(ValueError):
        ec.split_points(129)
    for n in (130, 514):
        r = ec.split_ranges(n)
        assert r == ec.split_ranges(n) and (64, 64) in r and r != sorted(r)
        covered = np.zeros(n, dtype=int)
        for a, b in r:
            covered[a:b] += 1
        assert (covered == 1).all() and len(r) == len(ec.split_points(n))


@pytest.mark.parametrize('kind', ec.KINDS)
def test_oracle_is_finite_at_every_size_and_configuration(kind):
    n_cases = 0
    for c in ec.size_cases():
        if c[0] != kind:
            continue
        cs = ec.case(*c)
        orc = ec.oracle(cs)
        eta = orc.wd_clip_state(cs['eta']) if cs['wd'] else cs['eta']
        ku, ke = orc.tendency(cs['uv'], eta, cs['dt'])
        u1, e1 = orc.ssprk33_step(cs['uv'], eta, cs['dt'])
        assert all(np.isfinite(x).all() for x in (ku, ke, u1, e1)), c
        assert np.abs(ku).max() > 0.0 and np.abs(e1 - eta).max() > 0.0, c
        if cs['wd']:
            if cs['mesh'].num_cells >= 62:
                assert 0.0 < ec.dry_share(cs) < 1.0, (c, ec.dry_share(cs))
        else:
            assert (cs['bath'][cs['mesh'].cells] + cs['eta']).min() > 0.0, c
        n_cases += 1
    assert n_cases == (65 if kind == 'tri' else 56)


@pytest.mark.parametrize('kind', ec.KINDS)
def test_oracle_tracer_is_finite_at_every_size(kind):
    for c in ec.tracer_cases():
        if c[0] != kind:
            continue
        cs = ec.case(*c, 'a')
        T, kw, _ = ec.tracer_setup(cs['mesh'], seed=31*c[1] + c[2])
        orc = ec.oracle(cs)
        k = orc.tracer_tendency(T, cs['uv'], cs['eta'], cs['dt'], **kw)
        T1 = orc.tracer_ssprk33_step(T, cs['uv'], cs['eta'], cs['dt'], **kw)
        lim = orc.limit(T)
        assert np.isfinite(k).all() and np.isfinite(T1).all() and np.isfinite(lim).all(), c
        assert np.abs(k).max() > 0.0, c
        assert cs['mesh'].num_cells < 62 or np.abs(lim - T).max() > 0.0, c


# ---- the range drivers on the C restatement -----------------------------------------------------------------------------------------
SPLIT_MESHES = [('tri', 13, 5), ('skew', 13, 10), ('warp', 13, 10)]


def _cpu_pair(kind, nx, ny, cfg, n_devices=2):
    cs = ec.case(kind, nx, ny, cfg)
    assert cs['mesh'].num_cells == 130
    T, _, ops = ec.tracer_setup(cs['mesh'], plain=True)
    devs = [ec.make_device(cs, CpuSwe2dDevice, reorder=None) for _ in range(n_devices)]
    return cs, T, devs, [ec.add_tracer(d, ops) for d in devs]


@pytest.mark.parametrize('cfg', ['a', 'b'])
@pytest.mark.parametrize('kind,nx,ny', SPLIT_MESHES)
def test_reference_ranges_give_the_bits_of_the_whole_launch(kind, nx, ny, cfg):
    cs, T, (whole, split), (tid_w, tid_s) = _cpu_pair(kind, nx, ny, cfg)
    ec.compare_split(whole, split, cs['uv'], cs['eta'], T, tid_w, tid_s, (kind, cfg))


@pytest.mark.parametrize('kind,nx,ny', SPLIT_MESHES)
def test_reference_leaves_cells_outside_a_range_untouched(kind, nx, ny):
    cs, T, (dev,), (tid,) = _cpu_pair(kind, nx, ny, 'a', n_devices=1)
    ec.check_outside_ranges(dev, tid, cs['uv'], cs['eta'], T, kind)


def test_the_checks_notice_a_wrong_range():
    """the drivers fail on a stand-in that is wrong the way a launch could be: a range that runs one cell too far, one that starts
    one cell late"""
    class TooFar(CpuSwe2dDevice):
        def solve_stage_cells(self, i, begin, end):
            CpuSwe2dDevice.solve_stage_cells(self, i, begin, min(end + 1, self.n_cells) if end > begin else end)

    class Late(CpuSwe2dDevice):
        def solve_stage_cells(self, i, begin, end):
            CpuSwe2dDevice.solve_stage_cells(self, i, begin + 1 if (begin == 64 and end == 65) else begin, end)

    cs = ec.case('tri', 13, 5, 'a')
    T, _, ops = ec.tracer_setup(cs['mesh'], plain=True)
    dev = ec.make_device(cs, TooFar, reorder=None)
    with pytest.raises(AssertionError, match='outside the range changed'):
        ec.check_outside_ranges(dev, ec.add_tracer(dev, ops), cs['uv'], cs['eta'], T)
    whole, split = ec.make_device(cs, CpuSwe2dDevice, reorder=None), ec.make_device(cs, Late, reorder=None)
    with pytest.raises(AssertionError, match='stage'):
        ec.compare_split(whole, split, cs['uv'], cs['eta'], T, ec.add_tracer(whole, ops), ec.add_tracer(split, ops))
