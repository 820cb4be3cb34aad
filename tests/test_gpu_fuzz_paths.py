"""GPU: the four ways a step is launched, over random option combinations on meshes of several tiles.

tests/test_gpu_fuzz.py draws every option of the shallow-water stage on 70 cells - one workgroup, no tile rings - and runs stage
launches and the dataflow kernel.  Here the same generator (tests/fuzz_cases.py, restricted to what the tile kernels of
csrc/swe2d_fuse.h cover) runs on the smallest meshes whose tiles have rings and neighbouring tiles, through the stage launches
(the yardstick), the fused stage pair, the three-stage kernel on tiles cut from the numbering and on caller patches: the same
call sequence on fresh devices - configuration, state, 3 steps, changed forcing, 2 steps (the three-stage kernel swaps two state
buffers per step: an odd and an even count) - must leave the same bits.  What is targeted are interactions no single-option test
sees: ring cells on boundaries of every kind, Function-valued boundary data read by ring lanes, boundary drag in the instances
without source terms (csrc/swe2d_handle.h has_sources() picks the instance and does not look at the boundaries), source-term
instances on rotated tiles.  A path that is not on is a failure, never a skip.

An error shared by every path would pass the bitwise comparison: the first step of the stage launches is also compared with the
numpy oracle, within the bound of tests/test_gpu_fuzz.py (set there at 70 cells, 400-878 here; every seed prints its figure, the
worst one belongs in profiles/r11a_path_fuzz.txt).  One oracle step takes 0.02-0.03 s at these sizes, general quadrilaterals
included, so every seed is compared."""
import numpy as np
import pytest

import fuzz_cases as fc
from helpers import make_oracle, make_oracle_generic, rel_linf
from test_gpu_fuzz import TOL

pytestmark = pytest.mark.gpu


def _oracle(c):
    mk = make_oracle_generic if c['quad'] else make_oracle
    return mk(c['mesh'], c['bath'], **c['o'])


def _device(c, mode):
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    o = c['o']
    dev = Swe2dDevice(c['mesh'], c['bath'], c['dt'], use_nonlinear_equations=o['use_nonlinear_equations'],
                      use_lax_friedrichs_velocity=o['use_lax_friedrichs_velocity'],
                      lax_friedrichs_velocity_scaling_factor=o['lax_friedrichs_velocity_scaling_factor'],
                      boundary_len=c['mesh'].boundary_len, reorder=c['reorder'])
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, mode)
    return dev


def _assert_path_on(dev, path, what):
    if path == 'pair':
        on, tiles, ring, _ = dev.fused_pair_info()
        assert on and tiles >= 3 and ring > 0, ('the fused stage pair is off', on, tiles, ring, what)
    elif path != 'stages':
        on, tiles, ring1, ring2 = dev.fused_triple_info()
        assert on and tiles >= 3 and ring1 > 0 and ring2 > 0, ('the three-stage kernel is off', on, tiles, ring1, ring2, what)


PATHS = {'stages': 0, 'pair': 1, 'triple': 3, 'triple_patches': 3}


def _run(c, path, what, first_step_only=False):
    """the call sequence every path runs; only SWE2D_OPT_FUSED_STAGES (and the caller's patches) differ"""
    from thetis_amd import ordering
    dev = _device(c, PATHS[path])
    try:
        if path == 'triple_patches':
            dev.fused_set_triple_tiles(*ordering.triple_tile_order(c['mesh'], *c['patch']))
        fc.apply_config(dev, c['dev_ops'], c['bcs'])
        dev.set_state(c['uv'], c['eta'])
        _assert_path_on(dev, path, what)
        if first_step_only:
            dev.advance(1)
            return dev.get_state()
        dev.advance(3)
        fc.apply_config(dev, c['ops2'], c['bcs2'])
        dev.advance(2)
        _assert_path_on(dev, path, what)
        return dev.get_state()
    finally:
        dev.close()


def _first_difference(c, a, b, ids=None):
    """where two states differ first: the cell in the caller's numbering (``ids``: the cells the rows stand for), and the markers
    of its boundary facets"""
    bad = np.nonzero((a[0] != b[0]).reshape(len(a[1]), -1).any(axis=1) | (a[1] != b[1]).any(axis=1))[0]
    if len(bad) == 0:
        return 'no cell differs'
    row = int(bad[0])
    cell = row if ids is None else int(ids[row])
    markers = [int(-m) for m in np.asarray(c['mesh'].cell_nbr)[cell] if m < 0]
    return '{} cells differ, the first is cell {} ({}; uv {} / {}, eta {} / {})'.format(
        len(bad), cell, 'boundary facets with markers {}'.format(markers) if markers else 'no boundary facet',
        a[0][row].ravel(), b[0][row].ravel(), a[1][row], b[1][row])


def _check_paths(c, paths):
    what = dict(seed=c['seed'], mesh=c['kind'], reorder=c['reorder'], patch=c['patch'], dt=c['dt'], options=fc.describe(c['o']),
                boundaries={m: {kk: ('field' if np.ndim(vv) >= 2 else vv) for kk, vv in f.items()} for m, f in c['bcs'].items()})
    # the first step of the stage launches against the oracle
    u1, e1 = _run(c, 'stages', what, first_step_only=True)
    uo, eo = _oracle(c).ssprk33_step(c['uv'], c['eta'], c['dt'])
    ru, re = rel_linf(u1, uo), rel_linf(e1, eo)
    print('PATHFUZZ oracle seed {} mesh {} rel_linf uv {:.3e} eta {:.3e}'.format(c['seed'], c['kind'], ru, re))
    assert ru < 10*TOL and re < 10*TOL, (ru, re, what)
    # the same bits by every path
    ref = _run(c, 'stages', what)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all(), what
    assert np.abs(ref[0] - c['uv']).max() > 0.0 and np.abs(ref[1] - c['eta']).max() > 0.0, what
    for path in paths:
        got = _run(c, path, what)
        assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (path, _first_difference(c, ref, got), what)


@pytest.mark.parametrize('seed', fc.TRI_SEEDS)
def test_fused_paths_give_the_bits_of_the_stage_launches_on_triangles(hip_lib, seed):
    """channel_case(24, 16) (768 cells: 4 tiles cut from the numbering, 16 under patches of 6 x 4 - every rotation), a ragged
    channel_case(29, 13) and Delaunay triangulations of ~400 points, by seed; device numbering, patch size and options drawn."""
    c = fc.path_case(seed)
    _check_paths(c, ['pair', 'triple'] + (['triple_patches'] if c['patch'] else []))


@pytest.mark.parametrize('seed', fc.QUAD_SEEDS)
def test_fused_pair_gives_the_bits_of_the_stage_launches_on_quadrilaterals(hip_lib, seed):
    """swe_fuse12_quad_kernel on skewed parallelograms, general cells and rectangles (its AFFINE and general instances)"""
    c = fc.quad_path_case(seed)
    assert c['mesh'].num_cells == fc.QUAD_NX*fc.QUAD_NY
    _check_paths(c, ['pair'])


def test_quadrilateral_mesh_is_the_smallest_of_three_tiles(hip_lib):
    """A tile holds at most 192 interior cells: 16 rows of 24 quadrilaterals (384 cells, row by row) are two full tiles, one more
    column makes three - in whatever numbering, which is what the fuzz above relies on."""
    from helpers import quad_case

    def tiles(nx, reorder):
        mesh, bath, uv, eta = quad_case(nx=nx, ny=fc.QUAD_NY, seed=0)
        c = dict(mesh=mesh, bath=bath, dt=0.5, reorder=reorder, o=dict(use_nonlinear_equations=True, use_lax_friedrichs_velocity=True,
                                                                       lax_friedrichs_velocity_scaling_factor=1.0))
        dev = _device(c, 1)
        try:
            dev.set_state(uv, eta)
            on, n_tiles, _, _ = dev.fused_pair_info()
            assert on
            return n_tiles
        finally:
            dev.close()
    assert tiles(fc.QUAD_NX - 1, None) == 2
    for reorder in fc.REORDERS:
        assert tiles(fc.QUAD_NX, reorder) >= 3, reorder


@pytest.mark.parametrize('seed', fc.PARTITION_SEEDS)
def test_three_stage_kernel_on_a_partition_range_with_random_options(hip_lib, seed):
    """swe2d_solve_step_cells(cell_end), cell_end inside the last or second-last tile, as tests/test_gpu_fuse3_rotation.py::
    test_stage_three_skips_cells_beyond_cell_end_on_every_lane does it without options: cells below cell_end get the bits of the
    stage launches on the same ranges, cells from cell_end on keep the marker written into the landing buffer beforehand.
    Structured meshes: caller patches, cell_end between two device numbers of the chosen patch (it then cuts through other patches
    as well); Delaunay meshes: tiles cut from the numbering (at most 256 cells each), cell_end up to 300 cells before the end."""
    from thetis_amd import ordering
    c = fc.partition_case(seed)
    mesh, uv, eta = c['mesh'], c['uv'], c['eta']
    n = mesh.num_cells
    marker = 7.25
    what = dict(seed=seed, mesh=c['kind'], reorder=c['reorder'], patch=c['patch'], options=fc.describe(c['o']))

    def run(fused, cell_end=None):
        dev = _device(c, 3 if fused else 0)
        try:
            perm = None if dev.perm is None else np.asarray(dev.perm)
            if cell_end is None:
                if c['patch']:
                    order, starts = ordering.triple_tile_order(mesh, *c['patch'])
                    bounds = list(starts) + [n]
                    t = len(starts) - c['tile_from_end']
                    cells = np.asarray(order[bounds[t]:bounds[t + 1]])
                    d = np.sort(cells if perm is None else np.asarray(dev.inv_perm)[cells])          # device numbers of the patch
                    cell_end = int(d[1 + int(c['frac']*(len(d) - 1))])
                    assert d[0] < cell_end <= d[-1]
                else:
                    cell_end = n - 1 - int(c['frac']*299)
            if fused and c['patch']:
                dev.fused_set_triple_tiles(*ordering.triple_tile_order(mesh, *c['patch']))
            fc.apply_config(dev, c['dev_ops'], c['bcs'])
            if fused:
                on, tiles, ring1, ring2 = dev.fused_step_info()
                assert on and tiles >= 3 and ring1 > 0 and ring2 > 0, (on, tiles, ring1, ring2, what)
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
            return dev.get_state(), perm, cell_end
        finally:
            dev.close()

    (u0, e0), perm, cell_end = run(False)
    (u3, e3), _, _ = run(True, cell_end)
    assert 0 < cell_end < n
    below = np.arange(n)[:cell_end] if perm is None else perm[:cell_end]     # caller's numbers of the device cells [0, cell_end)
    beyond = np.setdiff1d(np.arange(n), below)
    ref, got = (u0[below], e0[below]), (u3[below], e3[below])
    assert np.isfinite(e0[below]).all() and np.abs(e0[below] - eta[below]).max() > 0.0, what
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (cell_end, _first_difference(c, ref, got, below), what)
    assert (u3[beyond] == marker).all() and (e3[beyond] == marker).all(), (cell_end, what)
