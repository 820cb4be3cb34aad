"""The tide table on the device (csrc/swe2d_tide.hip): evaluation against the host expression, the batched advance against the
step-by-step path bit for bit and against the host-forced path, what the step plan reports, and FlowSolver2d's batches."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import rel_linf
from thetis_amd import _lib
from thetis_amd.device import FacetValues, Swe2dDevice, TideValues
from tide_cases import EPS, LX, LY, make_forcing, make_solver, run_tide_ranks, tide_mesh, _tide_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.3
# device against oracle / host for time-dependent boundary data, as tests/test_gpu_solver2d.py allows it
# (test_update_forcings_and_open_boundary, test_function_valued_tidal_boundary: rel_linf < 1e-10)
TOL_FORCED = 1e-10


def _bath(mesh):
    x, y = mesh.vertex_xy.T
    return 12.0 - 3.0*x/LX + 0.5*np.sin(y/900.0)


def _state(mesh, seed=3, depth=False):
    rng = np.random.default_rng(seed)
    n, k = mesh.cells.shape
    uv = 0.05*rng.normal(size=(n, k, 2))
    eta = 0.1*np.cos(np.pi*mesh.cell_xy()[:, :, 0]/LX) + 0.01*rng.normal(size=(n, k))
    return uv, eta


def _device(kind, K=3, wd=False, with_tide=True, manning=True):
    """a handle on the 8 x 4 mesh: the tide on marker 1, a constant normal velocity on marker 2"""
    mesh = tide_mesh(kind)
    dev = Swe2dDevice(mesh, _bath(mesh) - (11.5 if wd else 0.0), DT, boundary_len=mesh.boundary_len)
    f = make_forcing(mesh, K=K)
    if wd:
        dev.set_wetting_and_drying(0.5)
    if manning:
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    if with_tide:
        dev.tide_set([dev._slot(1)], f.omegas, *f.facet_tables(dev, 1))
        dev.set_bc(1, {'elev': TideValues()})
    dev.set_bc(2, {'un': 0.01})
    return mesh, dev, f


def _host_values(dev, mesh, f, t, marker=1):
    f.set_tidal_field(t)
    return dev.facet_node_values(marker, f.elev_field.dat.data_ro, cells_of_vertices=mesh.cells).values


# ---- 1. evaluation
@pytest.mark.parametrize('K', [1, 3, 32])
def test_evaluation_matches_set_tidal_field(hip_lib, K):
    """|device - host| <= (K + 4) eps (|mean| + sum_k |A_k|) per facet node.  Both sides evaluate
        s_0 = mean;  s_{k+1} = fl(s_k + fl(A_k * cos_x(fl(fl(omega_k t) - phi_k))))
    in the same order with no fused operation (contraction off on the device, numpy on the host), so the K arguments are identical
    bit for bit and the only difference is the cosine routine: each side's cosine is within 2 ulp of the true one, i.e. the two
    differ by at most 4 ulp(1)/2 = 2 eps, which enters the sum as 2 eps |A_k|, and after the rounding of the product as at most
    4 eps |A_k| - 'the 4'.  From then on the two sums carry different addends: each of the K additions rounds a partial sum that is
    bounded by |mean| + sum |A_k|, and the two roundings of a step differ by at most eps times that bound - 'the K'."""
    mesh, dev, f = _device('triangles', K=K)
    mean, amp, _ = f.facet_tables(dev, 1)
    bound = (K + 4)*EPS*(np.abs(mean) + np.abs(amp).sum(axis=0))
    for t in (0.0, 0.3, 44714.1, 2.6e6):
        dev.tide_eval(t)
        got = dev.tide_read()
        want = _host_values(dev, mesh, f, t)
        err = np.abs(got - want)
        print('K = {:d}  t = {:g}: max |device - host| = {:.3e}, bound {:.3e}'.format(K, t, err.max(), bound.min()))
        assert got.shape == want.shape == (4, 2) and np.isfinite(got).all()
        assert (err <= bound).all(), (K, t, float((err/bound).max()))
        assert np.abs(want).max() > 0.1
    dev.close()


@pytest.mark.parametrize('kind', ['triangles', 'quads'])
def test_other_marker_and_corner_cells_keep_their_values(hip_lib, kind):
    """marker 2 carries an elevation FIELD of its own (compact upload); the tide launches on marker 1 - whose end facets sit in
    corner cells that also own a facet of marker 2 (both corner quadrilaterals; of the triangles, cut along the left diagonal, the
    one at the origin) - leave every value of it alone, and the tide's own values stay when another table is set"""
    mesh, dev, f = _device(kind)
    s1, s2 = dev._slot(1), dev._slot(2)
    c1, _ = dev.boundary_facets(s1)
    c2, _ = dev.boundary_facets(s2)
    assert len(np.intersect1d(c1, c2)) == {'triangles': 1, 'quads': 2}[kind]      # cells that carry both markers
    mine = 7.0 + np.arange(2*len(c2), dtype=np.float64).reshape(len(c2), 2)
    dev.set_bc(2, {'elev': FacetValues(mine)})
    for t in (0.3, 44714.1):
        dev.tide_eval(t)
    tide = dev.tide_read()
    assert np.abs(tide - _host_values(dev, mesh, f, 44714.1)).max() < 1e-12
    # a table that lists marker 2's facets reads what the planes hold there (swe2d_tide_read gathers, swe2d_tide_set writes nothing)
    g = make_forcing(mesh, K=1, seed=5)
    dev.tide_set([s2], g.omegas, *g.facet_tables(dev, 2))
    assert np.array_equal(dev.tide_read(), mine)
    dev.tide_set([s1], f.omegas, *f.facet_tables(dev, 1))
    assert np.array_equal(dev.tide_read(), tide)
    dev.close()


# ---- 2. batched = step by step, bit for bit
T_BASE, K_FIRST, C = 0.7, 3, (0.0, 1.0, 0.5)


def _step_by_step(dev, n, forward_euler=False, tid=None):
    for k in range(n):
        t_k = T_BASE + (K_FIRST + k)*DT
        if forward_euler:
            dev.tide_eval(t_k + DT)
            dev.forward_euler_cells(0, dev.n_cells)
            dev.swap_state_buffers()
            continue
        for i in range(3):
            dev.tide_eval(t_k + C[i]*DT)
            dev.solve_stage(i)
        if tid is not None:
            for i in range(3):
                dev.tracer_solve_stage(tid, i)
            dev.tracer_limit(tid)


@pytest.mark.parametrize('case', ['triangles', 'quads', 'general', 'wetting_drying', 'forward_euler', 'tracer'])
def test_batched_advance_equals_step_by_step(hip_lib, case):
    kind = case if case in ('triangles', 'quads', 'general') else 'triangles'
    res = []
    for batched in (True, False):
        mesh, dev, f = _device(kind, wd=(case == 'wetting_drying'))
        uv, eta = _state(mesh)
        tid = None
        if case == 'tracer':
            tid = dev.add_tracer()
            dev.tracer_set_state(tid, 1.0 + (mesh.cell_xy()[:, :, 0] > 0.5*LX))
            dev.tracer_set_bc(tid, 1, 1.5)
        dev.set_state(uv, eta)
        if batched:
            dev.tide_clock(T_BASE, K_FIRST)
            if case == 'forward_euler':
                dev.advance_forward_euler(5)
            elif case == 'tracer':
                dev.advance_coupled(5, use_limiter=True)
            else:
                dev.advance(2)
                dev.advance(3)                                         # the library counts the steps on
        else:
            _step_by_step(dev, 5, forward_euler=(case == 'forward_euler'), tid=tid)
        res.append(dev.get_state() + (dev.tide_read(),) + ((dev.tracer_get_state(tid),) if tid is not None else ()))
        last = T_BASE + (K_FIRST + 4)*DT
        want = _host_values(dev, mesh, f, last + DT if case == 'forward_euler' else last + 0.5*DT)
        assert np.abs(res[-1][2] - want).max() < 1e-12                 # the last stage of the last step was evaluated at its time
        dev.close()
    for a, b in zip(*res):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    uv0, eta0 = _state(tide_mesh(kind))
    assert np.abs(res[0][1] - eta0).max() > 1e-4                        # (the steps moved the state)


# ---- 3. against the host-forced path
def test_batched_advance_against_host_forced_path(hip_lib):
    """20 steps of the batched run of (2) against the existing path: ``set_tidal_field`` on the host at every stage time, the
    compact upload (swe2d_set_bc_facets), one stage launch.  The tolerance is the suite's own for time-dependent boundary data
    between the device and its oracles (tests/test_gpu_solver2d.py: rel_linf < 1e-10)."""
    mesh, dev, f = _device('triangles')
    uv, eta = _state(mesh)
    dev.set_state(uv, eta)
    dev.tide_clock(T_BASE, K_FIRST)
    dev.advance(20)
    ua, ea = dev.get_state()
    dev.close()
    mesh, host, f = _device('triangles', with_tide=False)
    host.set_state(uv, eta)
    for k in range(20):
        t_k = T_BASE + (K_FIRST + k)*DT
        for i in range(3):
            f.set_tidal_field(t_k + C[i]*DT)
            host.set_bc(1, {'elev': host.facet_node_values(1, f.elev_field.dat.data_ro, cells_of_vertices=mesh.cells)})
            host.solve_stage(i)
    ub, eb = host.get_state()
    host.close()
    print('device tide against host-forced path after 20 steps: rel_linf eta {:.3e}, uv {:.3e}'.format(rel_linf(ea, eb), rel_linf(ua, ub)))
    assert rel_linf(ea, eb) < TOL_FORCED and rel_linf(ua, ub) < TOL_FORCED
    assert np.abs(ea - eta).max() > 1e-3


# ---- 4. plan
def _plan(dev):
    return dev.fused_pair_info(), dev.fused_triple_info(), dev.fused_step_info(), dev.flow_supported()


@pytest.mark.parametrize('fused', [None, 3])
def test_plan_declines_a_tide(hip_lib, fused):
    mesh, fresh, _ = _device('triangles', with_tide=False, manning=False)
    mesh, dev, f = _device('triangles', manning=False)
    for d in (fresh, dev):
        if fused is not None:
            d.set_option(_lib.OPT_FUSED_STAGES, fused)
            d.set_option(_lib.OPT_FLOW, 0)
    want = _plan(fresh)
    assert want[3] == 2 and (fused is None or (want[1][0] and want[2][0]))
    got = _plan(dev)
    assert not got[0][0] and not got[1][0] and not got[2][0] and got[3] == 0
    for call in (lambda: dev.solve_flow([mesh.num_cells]*3), lambda: dev.solve_step_cells(mesh.num_cells),
                 lambda: dev.solve_stage_pair_cells(mesh.num_cells, mesh.num_cells)):
        with pytest.raises(_lib.Swe2dError) as err:
            call()
        assert err.value.code == _lib.ERR_UNSUPPORTED
    dev.tide_clear()
    dev.set_bc(1, None)
    assert _plan(dev) == want
    fresh.close()
    dev.close()


def test_advance_inside_a_capture_is_refused(hip_lib):
    import torch
    mesh, dev, f = _device('triangles')
    mesh, twin, _ = _device('triangles')
    uv, eta = _state(mesh)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev.set_state(uv, eta)
        buf = torch.zeros(16, device='cuda')
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            buf.add_(1.0)                                               # (the capture records something; nothing is replayed)
            for call in (lambda: dev.advance(1), lambda: dev.advance_forward_euler(1), lambda: dev.tide_eval(1.0)):
                with pytest.raises(_lib.Swe2dError) as err:
                    call()
                assert err.value.code == _lib.ERR_UNSUPPORTED
        s.synchronize()
        dev.tide_clock(T_BASE, K_FIRST)                                 # the handle is usable: the refused calls left the clock alone
        dev.advance(2)
        ua, ea = dev.get_state()
    dev.set_stream(None)
    twin.set_state(uv, eta)
    twin.tide_clock(T_BASE, K_FIRST)
    twin.advance(2)
    ub, eb = twin.get_state()
    assert np.isfinite(ea).all() and np.array_equal(ea, eb) and np.array_equal(ua, ub)
    dev.close()
    twin.close()


# ---- 5. solver
def _solver_run(tmp_path, batched):
    from thetis_amd import DetectorsCallback
    from thetis_amd.rungekutta import SSPRK33
    calls = []
    orig = SSPRK33.advance_steps

    def counting(self, t, n, probes=None, clock=None):
        calls.append((n, clock))
        return orig(self, t, n, probes=probes, clock=clock)
    SSPRK33.advance_steps = counting
    try:
        mesh = tide_mesh('triangles')
        s = make_solver(mesh, make_forcing(mesh, K=3), dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path))
        assert s.timestepper.wants_clock and not s.timestepper.forced_per_stage
        s.add_callback(DetectorsCallback(s, [(0.3*LX, 0.4*LY), (0.8*LX, 0.7*LY)], ['elev_2d', 'uv_2d'], 'gauges'), 'timestep')
        if batched:
            s.iterate()
        else:
            for _ in s.create_iterator():
                pass
        cb = s.callbacks['timestep']['gauges']
        return (s.fields.elev_2d.dat.data_ro.copy(), s.fields.uv_2d.dat.data_ro.copy(), [h[0] for h in cb.history],
                np.array([h[1] for h in cb.history]), s.simulation_time, s.iteration, calls)
    finally:
        SSPRK33.advance_steps = orig


def test_iterate_batches_a_tidally_forced_run(hip_lib, tmp_path):
    a = _solver_run(tmp_path / 'a', True)
    assert a[6] == [(4, (0.0, 0)), (4, (0.0, 4))]                       # one advance_steps per export interval, the loop's clock
    b = _solver_run(tmp_path / 'b', False)
    assert b[6] == []
    assert a[4] == b[4] and a[5] == b[5] == 8 and a[2] == b[2] and len(a[2]) == 8
    for x, y in zip(a[:2] + (a[3],), b[:2] + (b[3],)):
        assert np.isfinite(x).all() and np.array_equal(x, y)
    # the tide drove it: a boundary at rest ends elsewhere
    from thetis_amd import Constant
    c = make_solver(tide_mesh('triangles'), Constant(0.0), dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path / 'c'))
    c.iterate()
    assert np.abs(c.fields.elev_2d.dat.data_ro - a[0]).max() > 1e-6


def test_two_ranks_take_the_host_path(hip_lib, tmp_path):
    """several ranks: every rank evaluates the tide on the host per stage (DESIGN.md "Tidal boundary forcing") - the single-rank,
    device-evaluated state within the tolerance of test 3, nothing raised"""
    single = _tide_case(str(tmp_path / 'one'))
    assert single.timestepper.wants_clock
    e1, u1 = single.fields.elev_2d.dat.data_ro.copy(), single.fields.uv_2d.dat.data_ro.copy()
    ranks = run_tide_ranks(2, str(tmp_path))
    for r in ranks:
        assert r['iteration'] == single.iteration == 20 and r['simulation_time'] == single.simulation_time
        print('two ranks against one: rel_linf eta {:.3e}, uv {:.3e}'.format(rel_linf(r['elev'], e1), rel_linf(r['uv'], u1)))
        assert rel_linf(r['elev'], e1) < TOL_FORCED and rel_linf(r['uv'], u1) < TOL_FORCED


# ---- 6. the example
def test_tidal_channel_example(hip_lib):
    r = subprocess.run([sys.executable, os.path.join('examples', 'tidal_channel.py'), '--nx', '8', '--ny', '4', '--t-end', '200', '--farm'],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    last = lines[-2].split()
    assert last[0] == 'steps' and int(last[1]) >= 10
    vals = [float(last[i]) for i in (3, 6, 9)]
    assert np.isfinite(vals).all() and vals[1] > 0.0 and vals[2] > 0.0
    g = lines[-1].split()
    assert g[0] == 'gauge' and int(g[2]) == int(last[1]) and np.isfinite(float(g[5]))
