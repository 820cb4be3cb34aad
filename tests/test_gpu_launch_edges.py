"""GPU: the stage kernels at mesh sizes on the edges of a wave, a workgroup and a tile, and on arbitrary cell ranges (tests/edge_cases.py
holds the meshes, the configurations and the range drivers; tests/test_edge_cases.py runs the drivers on the references alone).

A  every size and configuration against the numpy oracle within the bounds of tests/test_gpu_fuzz.py - tendency rel_linf < TOL =
   2e-12 (that file's scale rule for the eta tendency), a step < 10*TOL - by three ``solve_stage`` calls, ``advance(1)`` under the plan,
   SWE2D_OPT_FUSED_STAGES forced to 0 / 1 / 3 without the dataflow kernel wherever csrc/swe2d_plan.hip step_kernels() covers the handle,
   and ``solve_flow``; every one of them the bits of the stage launches, the path asserted through ``fused_*_info()``.  The tracer stage
   and the vertex limiter likewise (bounds of test_random_tracer_option_combinations_match_oracle and test_limiter_matches_oracle).
B  ``solve_stage_cells`` / ``forward_euler_cells`` / ``tracer_solve_stage_cells`` / ``tracer_limit_cells`` range by range
   (edge_cases.split_ranges: cuts at 1, 63, 64, 65, 127, 129, n - 1, an empty range, shuffled) give the bits of one launch over [0, n),
   under every option that changes what a launch does with its range.
C  cells outside a range keep their bits.
D  empty and invalid ranges.

Forced modes below 64 cells: step_plan() of csrc/swe2d_plan.hip takes a forced tile kernel from kForcedFromCells = 64 cells, so on the
three sizes below (2, 6, 62 triangles; 1, 2, 63 quadrilaterals) a forced mode must report the stage launches - asserted, on both sides of
the constant (62 | 64 triangles, 63 | 64 quadrilaterals); the step is compared all the same.  No size is excluded for any path.

``python tests/test_gpu_launch_edges.py FILE`` writes the table of measured errors to FILE."""
import os
import sys

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import edge_cases as ec
from helpers import rel_linf
from thetis_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 2e-12                             # tests/test_gpu_fuzz.py
TOL_LIMITER = 1e-14                     # tests/test_gpu_tracer.py::test_limiter_matches_oracle
PATHS = {'stages': 0, 'pair': 1, 'triple': 3}
FORCED_FROM_CELLS = 64                  # csrc/swe2d_plan.hip kForcedFromCells
SIZE_CASES = ec.size_cases()
TRACER_CASES = ec.tracer_cases()


def _device(cs, reorder):
    from thetis_amd.device import Swe2dDevice
    dev = ec.make_device(cs, Swe2dDevice, reorder)
    _own_rules(dev)
    return dev


def _own_rules(dev):
    for opt in (_lib.OPT_FUSED_STAGES, _lib.OPT_FLOW, _lib.OPT_FLOW_WD, _lib.OPT_BND_INLINE, _lib.OPT_LDSX, _lib.OPT_ALTERNATE,
                _lib.OPT_COMPACT_IDX, _lib.OPT_VISC_FUSION):
        dev.set_option(opt, None)       # the handle's own rule unless a case says otherwise (not the environment)


def _covers(cs, path):
    """csrc/swe2d_plan.hip step_kernels(): `if (h->wd) k &= ... kFlow : 0u`, `if (h->visc) k = 0`, quadrilaterals the pair alone"""
    if path == 'stages':
        return True
    return not cs['wd'] and 'horizontal_viscosity' not in cs['o'] and (path == 'pair' or not cs['quad'])


def _assert_path(dev, path, n, what):
    pair, triple = dev.fused_pair_info(), dev.fused_triple_info()
    if path == 'stages':
        assert not pair[0] and not triple[0], ('a fused kernel is on where stage launches were asked for', what)
        return
    on, tiles = (pair if path == 'pair' else triple)[:2]
    if n >= FORCED_FROM_CELLS:
        assert on and tiles >= 1, ('the forced {} is off'.format(path), on, tiles, what)
    else:                               # step_plan(): n >= kForcedFromCells
        assert not on, ('the forced {} is on below kForcedFromCells'.format(path), on, tiles, what)


def check_sizes(c, reorder, log=None):
    cs = ec.case(*c)
    mesh, uv, eta, dt = cs['mesh'], cs['uv'], cs['eta'], cs['dt']
    n = mesh.num_cells
    what = (ec.case_id(c), reorder)
    orc = ec.oracle(cs)
    dev = _device(cs, reorder)
    try:
        dev.set_state(uv, eta)
        if cs['wd']:
            eta = orc.wd_clip_state(eta)     # what set_state does on the device: nodal depths through the positivity limiter
        ku, ke = dev.tendency()
        ku_o, ke_o = orc.tendency(uv, eta, dt)
        scale = max(np.abs(ke_o).max(), 1e-12*np.abs(ku_o).max())      # (with wetting-drying: the tendency of zeta = D - h)
        err_t = max(rel_linf(ku, ku_o), float(np.abs(ke - ke_o).max()/max(scale, 1e-300)))
        print('EDGES {} {} tendency {:.3e}'.format(*what, err_t))
        uo, eo = orc.ssprk33_step(uv, eta, dt)
        worst = [0.0]

        def step(got, how, ref=None):
            err = max(rel_linf(got[0], uo), rel_linf(got[1], eo))
            print('EDGES {} {} step by {} {:.3e}'.format(*what, how, err))
            worst[0] = max(worst[0], err)
            assert err < 10*TOL, (how, err, what)
            if ref is not None:
                assert ec.same_bits(ref, got), (how, ec.first_difference(ref, got), what)

        assert rel_linf(ku, ku_o) < TOL, what
        assert np.abs(ke - ke_o).max() < TOL*max(scale, 1e-300), what
        dev.set_state(uv, cs['eta'])
        for i in range(3):
            dev.solve_stage(i)
        ref = dev.get_state()
        step(ref, 'solve_stage x 3')
        dev.set_state(uv, cs['eta'])
        dev.advance(1)
        step(dev.get_state(), 'advance(1)', ref)
        for path, mode in PATHS.items():
            if not _covers(cs, path):
                continue
            dev.set_option(_lib.OPT_FLOW, 0)
            dev.set_option(_lib.OPT_FUSED_STAGES, mode)
            dev.set_state(uv, cs['eta'])
            _assert_path(dev, path, n, what)
            dev.advance(1)
            _assert_path(dev, path, n, what)
            step(dev.get_state(), 'forced ' + path, ref)
        dev.set_option(_lib.OPT_FLOW, None)
        dev.set_option(_lib.OPT_FUSED_STAGES, None)
        if dev.flow_supported():
            dev.set_state(uv, cs['eta'])
            dev.solve_flow([n]*3)
            assert dev.flow_timeouts() == 0, what
            step(dev.get_state(), 'solve_flow', ref)
        if log is not None:
            log.append((c, err_t, worst[0]))
    finally:
        dev.close()


def _reorder(index):
    return 'hilbert' if index % 2 else 'auto'


# ---- A. sizes against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', SIZE_CASES, ids=ec.case_id)
def test_sizes_match_oracle_by_every_path(hip_lib, c):
    check_sizes(c, _reorder(SIZE_CASES.index(c)))


def test_forced_paths_are_asked_for_on_both_sides_of_64_cells():
    """what the size cases rely on, without a device: each forced path is asked for on both sides of 64 cells, for both cell types"""
    for path in ('pair', 'triple'):
        ns = {(cs['quad'], cs['mesh'].num_cells) for cs in (ec.case(*c) for c in SIZE_CASES) if _covers(cs, path)}
        assert {(False, 62), (False, 64), (False, 514)} <= ns
        assert ({(True, 63), (True, 64), (True, 257)} <= ns) == (path == 'pair')


@pytest.mark.parametrize('c', TRACER_CASES, ids=ec.case_id)
def test_tracer_sizes_match_oracle(hip_lib, c):
    index = TRACER_CASES.index(c)
    cs = ec.case(*c, 'a')
    uv, eta, dt = cs['uv'], cs['eta'], cs['dt']
    T, kw, ops = ec.tracer_setup(cs['mesh'], seed=31*c[1] + c[2])
    orc = ec.oracle(cs)
    what = (ec.case_id(c), _reorder(index))
    dev = _device(cs, _reorder(index))
    try:
        tid = ec.add_tracer(dev, ops)
        dev.set_state(uv, eta)
        dev.tracer_set_state(tid, T)
        err_t = rel_linf(dev.tracer_tendency(tid), orc.tracer_tendency(T, uv, eta, dt, **kw))
        for i in range(3):
            dev.tracer_solve_stage(tid, i)
        err_s = rel_linf(dev.tracer_get_state(tid), orc.tracer_ssprk33_step(T, uv, eta, dt, **kw))
        dev.tracer_set_state(tid, T)
        dev.tracer_limit(tid)
        err_l = rel_linf(dev.tracer_get_state(tid), orc.limit(T))
        print('EDGES {} {} tracer tendency {:.3e} step {:.3e} limiter {:.3e}'.format(*what, err_t, err_s, err_l))
        assert err_t < TOL and err_s < 10*TOL and err_l < TOL_LIMITER, (err_t, err_s, err_l, what)
    finally:
        dev.close()


# ---- B. ranges give the bits of the whole launch ------------------------------------------------------------------------------------
def _turbine_params(projected_diameter):
    p = _lib.TurbineParams()
    p.rotor_area = np.pi*30.0**2
    p.projected_diameter = projected_diameter
    p.thrust_area_const = 0.8*p.rotor_area
    p.power_const = 0.4
    p.rho0 = 1000.0
    return p


def _discrete_farm(dev, mesh):
    """a discrete farm as tests/test_gpu_discrete_turbines.py builds one: bumps of 3 km radius (1.5 cells), one across the boundary, two
    overlapping, one across the edge of the farm's subdomain (x_c < 20 km of the 26 km)"""
    import discrete_turbine_ref as dr
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    phi, w = dr.rule(3, 10)
    dev.dfarm_set(0, _turbine_params(6e3), [[6e3, 5e3], [12e3, 4e3], [14e3, 6e3], [20e3, 5e3], [9e3, 0.5e3]], xc < 20e3, phi, w)
    cells, dens = dev.dfarm_density_read(0)
    d = np.sort(cells if dev.perm is None else np.asarray(dev.inv_perm)[cells])
    assert (dens > 0.0).any() and d[0] < 63 and d[-1] > 65, 'the farm does not reach across the cuts'


def _continuous_farm(dev, mesh):
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    dev.turbine_farm_set(0, _turbine_params(18.0), np.where(((xc > 4e3) & (xc < 22e3))[:, None], 1e-5, 0.0)*np.ones((1, 3)))


# id -> (configuration, viscosity on top, options, what else to set on the device)
TRI_SETUPS = {
    'a': ('a', False, {}, None),
    'a-bnd_inline_0': ('a', False, {_lib.OPT_BND_INLINE: 0}, None),
    'a-ldsx_1': ('a', False, {_lib.OPT_LDSX: 1}, None),
    'a-alternate_1': ('a', False, {_lib.OPT_ALTERNATE: 1}, None),
    'a-compact_idx_2': ('a', False, {_lib.OPT_COMPACT_IDX: 2}, None),
    'd-visc_fusion_1': ('d', False, {_lib.OPT_VISC_FUSION: 1}, None),
    'd-visc_fusion_0': ('d', False, {_lib.OPT_VISC_FUSION: 0}, None),
    'c': ('c', False, {}, None),
    'c-viscosity': ('c', True, {}, None),
    'a-discrete_farm': ('a', False, {}, _discrete_farm),
    'a-continuous_farm': ('a', False, {}, _continuous_farm),
}
QUAD_SETUPS = {'a': ('a', False, {}, None), 'c': ('c', False, {}, None), 'd': ('d', False, {}, None)}
SPLIT_CASES = [('tri', 13, 5, s) for s in TRI_SETUPS] + [(kind, 13, 10, s) for kind in ec.QUAD_GEOMETRIES for s in QUAD_SETUPS]


def _setup_case(kind, nx, ny, setup):
    cfg, visc, options, extra = (TRI_SETUPS if kind == 'tri' else QUAD_SETUPS)[setup]
    cs = ec.case(kind, nx, ny, cfg)
    assert cs['mesh'].num_cells == ec.SPLIT_FROM
    if visc:
        cs = dict(cs, o=dict(cs['o']), dev_ops=list(cs['dev_ops']))
        ec.add_viscosity(cs['mesh'], cs['o'], cs['dev_ops'])
    return cs, options, extra


def _setup_device(cs, options, extra, reorder):
    dev = _device(cs, reorder)
    for opt, value in options.items():
        dev.set_option(opt, value)
    if _lib.OPT_COMPACT_IDX in options:
        assert dev.connectivity_info()[0] == 1, 'the 16-byte connectivity records are not in use'
    if extra is not None:
        extra(dev, cs['mesh'])
    return dev


@pytest.mark.parametrize('reorder', [None, 'hilbert'])
@pytest.mark.parametrize('kind,nx,ny,setup', SPLIT_CASES, ids=[ec.case_id(c) for c in SPLIT_CASES])
def test_ranges_give_the_bits_of_the_whole_launch(hip_lib, kind, nx, ny, setup, reorder):
    cs, options, extra = _setup_case(kind, nx, ny, setup)
    T, _, ops = ec.tracer_setup(cs['mesh'])
    devs = []
    try:
        for _ in range(2):
            devs.append(_setup_device(cs, options, extra, reorder))
        tids = [ec.add_tracer(d, ops) for d in devs]
        ec.compare_split(devs[0], devs[1], cs['uv'], cs['eta'], T, tids[0], tids[1], (kind, setup, reorder))
    finally:
        for d in devs:
            d.close()


# ---- C. cells outside a range keep their bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('reorder', [None, 'hilbert'])
@pytest.mark.parametrize('kind,nx,ny', [('tri', 13, 5), ('skew', 13, 10), ('warp', 13, 10)])
def test_cells_outside_a_range_keep_their_bits(hip_lib, kind, nx, ny, reorder):
    """configuration (a), where set_state / get_state is exact (include/swe2d.h: not with wetting-drying, the device carries D)"""
    cs = ec.case(kind, nx, ny, 'a')
    T, _, ops = ec.tracer_setup(cs['mesh'])
    dev = _device(cs, reorder)
    try:
        assert (dev.perm is None) == (reorder is None)
        tid = ec.add_tracer(dev, ops)
        ec.check_outside_ranges(dev, tid, cs['uv'], cs['eta'], T, (kind, reorder))
    finally:
        dev.close()


# ---- D. argument edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,nx,ny', [('tri', 13, 5), ('warp', 13, 10)])
def test_empty_and_invalid_ranges(hip_lib, kind, nx, ny):
    """Every range below is turned down on the host before anything is launched: swe2d_solve_stage_cells, swe2d_forward_euler_cells and
    swe2d_tracer_solve_stage_cells test `cell_begin < 0 || cell_end > n_cells || cell_begin > cell_end` first, swe2d_tracer_limit_cells
    `cell_end < 0 || cell_end > n_cells` (limiter_apply, csrc/swe2d_api_tracer.hip); an empty range returns before the launch."""
    cs = ec.case(kind, nx, ny, 'a')
    T, _, ops = ec.tracer_setup(cs['mesh'])
    n = cs['mesh'].num_cells
    dev = _device(cs, 'hilbert')
    try:
        tid = ec.add_tracer(dev, ops)
        dev.set_state(cs['uv'], cs['eta'])
        dev.tracer_set_state(tid, T)
        for i in range(3):
            dev.solve_stage(i)
            dev.tracer_solve_stage(tid, i)

        def everything():
            return [dev.get_state(i) for i in range(3)] + [(dev.tracer_get_buffer(tid, b),) for b in range(3)]

        before = everything()
        calls = [lambda a, b, i=i: dev.solve_stage_cells(i, a, b) for i in range(3)]
        calls += [lambda a, b, i=i: dev.tracer_solve_stage_cells(tid, i, a, b) for i in range(3)]
        calls += [lambda a, b: dev.forward_euler_cells(a, b)]
        bad = [(65, 64), (n, 0), (-1, 64), (-1, -1), (0, n + 1), (n, n + 1), (n + 1, n + 1)]
        for call in calls[:6]:
            for a in (0, 64, n):
                call(a, a)                                   # returns SWE2D_OK (a failure raises)
            for a, b in bad:
                with pytest.raises(_lib.Swe2dError) as err:
                    call(a, b)
                assert err.value.code == _lib.ERR_INVALID_ARGUMENT, (a, b)
        for m in (-1, n + 1):
            with pytest.raises(_lib.Swe2dError) as err:
                dev.tracer_limit_cells(tid, m)
            assert err.value.code == _lib.ERR_INVALID_ARGUMENT, m
        dev.tracer_limit_cells(tid, 0)                        # the empty range of the limiter: the bounds are formed, nothing is written
        for ref, got in zip(before, everything()):
            assert ec.same_bits(ref, got)
        # ForwardEuler last: also an empty step invalidates the stage solutions (swe2d_forward_euler_cells), the state stays
        for a, b in bad:
            with pytest.raises(_lib.Swe2dError) as err:
                calls[6](a, b)
            assert err.value.code == _lib.ERR_INVALID_ARGUMENT, (a, b)
        for a in (0, 64, n):
            calls[6](a, a)
        assert ec.same_bits(before[2], dev.get_state()) and ec.same_bits(before[3], (dev.tracer_get_state(tid),))
    finally:
        dev.close()


# ---- the table of measured errors ---------------------------------------------------------------------------------------------------
def error_table():
    lines = ['# worst error of the HIP kernels against the numpy oracle over the sizes of tests/edge_cases.py, as rel_linf (bounds: tendency',
             '# 2e-12, step 2e-11) and in units of eps = 2^-52; step: the worst of solve_stage x 3, advance(1), the forced paths and solve_flow',
             '# {:<14s} {:>4s} {:>6s} {:>12s} {:>8s} {:>10s} {:>12s} {:>8s} {:>10s}'.format(
                 'cells', 'cfg', 'sizes', 'tendency', 'eps', 'at', 'step', 'eps', 'at')]
    log = []
    for index, c in enumerate(SIZE_CASES):
        check_sizes(c, _reorder(index), log)
    eps = np.finfo(np.float64).eps
    for kind in ec.KINDS:
        for cfg in ec.CONFIGS:
            rows = [r for r in log if r[0][0] == kind and r[0][3] == cfg]
            t = max(rows, key=lambda r: r[1])
            s = max(rows, key=lambda r: r[2])
            name = {'tri': 'triangles', 'skew': 'parallelograms', 'warp': 'general quads'}[kind]
            lines.append('{:<16s} {:>4s} {:>6d} {:>12.3e} {:>8.1f} {:>10s} {:>12.3e} {:>8.1f} {:>10s}'.format(
                name, cfg, len(rows), t[1], t[1]/eps, '{}x{}'.format(*t[0][1:3]), s[2], s[2]/eps, '{}x{}'.format(*s[0][1:3])))
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    with open(sys.argv[1], 'w') as fh:
        fh.write(error_table())
