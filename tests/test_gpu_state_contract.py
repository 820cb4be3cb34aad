"""The host bookkeeping around the step kernels, against a model: which physical buffer is state buffer A, which stage solutions
swe2d_get_stage_state may hand out, and what a captured graph reads when it is replayed.

Every stepping path of Swe2dDevice (stage launches, fused stage pair, three-stage kernel, dataflow kernel, quadrilaterals,
wetting-drying, coupled SWE + tracer) is driven by a seeded random sequence of operations - steps of odd and even counts, stage
launches with reads in between, ForwardEuler steps whole-mesh and by ranges, new states, captured and replayed step sequences -
next to a handle that runs the same sequence by plain stage launches.  Every read either equals the model (SSPRK33 in Shu-Osher
form on the numpy oracle's tendency, coefficients of tests/golden/shuosher_ssprk33.json) to 1e-11 and has the bits of the
stage-launch handle, or is refused with SWE2D_ERR_UNSUPPORTED - never anything else.  The second half pins the defects of this
bookkeeping one by one."""
import json
import os
import types

import numpy as np
import pytest

from helpers import channel_case, make_oracle, make_ref, quad_case, rel_linf

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(_HERE, 'golden', 'shuosher_ssprk33.json')) as _f:
    _SO = json.load(_f)
ALPHA = [[float.fromhex(v) for v in row] for row in _SO['alpha_hex']]
BETA = [[float.fromhex(v) for v in row] for row in _SO['beta_hex']]
TOL = 1e-11
TOL_TRACER = 1e-10        # tracer + limiter after the SWE step (test_gpu_tracer.test_coupled_steps_match_cpu_restatement)
DT = 2.0


class Model(object):
    """What the handle's state and stage buffers must hold: U, and U(1), U(2) of the step made last with a flag each for
    "the contract lets swe2d_get_stage_state hand it out"; optionally one tracer (RefTracer + limiter)."""

    def __init__(self, orc, wd=False, tracer=None):
        self.orc, self.wd, self.rt = orc, wd, tracer
        self.u = self.e = None
        self.s = [None, None]
        self.valid = [False, False]
        self.last = None                   # 'advance': a step of swe2d_advance's choice (fused / flow paths keep stages on chip)
        self.T = None

    def set_state(self, uv, eta):
        self.u, self.e = uv.copy(), (self.orc.wd_clip_state(eta) if self.wd else eta.copy())
        self.valid = [False, False]
        self.last = None

    def stages(self, u, e):
        """[(U1), (U2), (U3)] of one SSPRK33 step from (u, e) (oracle.swe2d_oracle.SWEOracle.ssprk33_step, stages kept)."""
        orc = self.orc
        su, se = [u], [e]
        sol_u, sol_e = u, e
        out = []
        for i in range(3):
            k_u, k_e = orc.tendency(sol_u, sol_e, DT)
            new_u, new_e = k_u*BETA[i + 1][i], k_e*BETA[i + 1][i]
            for j in range(i + 1):
                new_u = new_u + su[j]*ALPHA[i + 1][j]
                new_e = new_e + ((orc.nodal_depth(se[j]) - orc.h) if self.wd else se[j])*ALPHA[i + 1][j]
            if self.wd:
                new_u, new_e = orc.wd_finish_stage(new_u, new_e, BETA[i + 1][i]*DT)
            sol_u, sol_e = new_u, new_e
            su.append(sol_u); se.append(sol_e)
            out.append((sol_u, sol_e))
        return out

    def step(self, kind='advance'):
        (u1, e1), (u2, e2), (u3, e3) = self.stages(self.u, self.e)
        self.s = [(u1, e1), (u2, e2)]
        self.valid = [True, True]
        self.u, self.e = u3, e3
        self.last = kind

    def stage(self, i):
        """solve_stage(i) alone (in order 0, 1, 2: the step's input is U while stage 2 has not run)"""
        if i == 0:
            self._pending = self.stages(self.u, self.e)
        if i < 2:
            self.s[i] = self._pending[i]
            self.valid[i] = True
        else:
            self.u, self.e = self._pending[2]
        self.last = 'stages'

    def forward_euler(self):
        self.u, self.e = self.orc.forward_euler_step(self.u, self.e, DT)
        self.valid = [False, False]
        self.last = None

    def coupled(self):
        self.step()
        self.T = self.rt.limit(self.rt.step(self.T, self.u, DT))

    def captured(self):
        """after a capture: the stage buffers are rewritten by replays the host does not see"""
        self.valid = [False, False]
        self.last = None

    def read(self, i):
        return (self.u, self.e) if i == 2 else self.s[i]


def _check_read(dev, base, model, i, path):
    from thetis_amd import _lib
    try:
        got = dev.get_state(i)
    except _lib.Swe2dError as err:
        assert err.code == _lib.ERR_UNSUPPORTED, str(err)
        # a fused / dataflow step keeps U(1) (and U(2)) on chip; stage launches and plain reads must answer
        may = i < 2 and model.last == 'advance' and path != 'stages'
        assert not (i == 2 or model.valid[i]) or may, 'read {:d} refused although it is in memory: {:}'.format(i, err)
        return
    assert i == 2 or model.valid[i], 'stage {:d} handed out although no launch of the last step left it in memory'.format(i)
    want = model.read(i)
    assert rel_linf(got[0], want[0]) < TOL and rel_linf(got[1], want[1]) < TOL, \
        (i, rel_linf(got[0], want[0]), rel_linf(got[1], want[1]))
    ref = base.get_state(i)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), 'not the bits of the stage launches (read {:d})'.format(i)


def _case(path, seed):
    """(mesh, bath, first state, state maker, oracle kwargs, wetting-drying alpha or None)"""
    if path == 'quad':
        mesh, bath, uv, eta = quad_case(nx=30, ny=16, seed=seed, amp_eta=0.3, amp_u=0.2)
    elif path == 'wd':
        from thetis_amd.mesh import RectangleMesh
        lx, ly = 13800.0, 7200.0                                   # tests/test_wetting_drying.py: a beach, dry for x < 2760 m
        mesh = RectangleMesh(24, 12, lx, ly)
        x, y = mesh.vertex_xy.T
        bath = x/2760.0 - 1.0
        alpha = 0.3 + 0.2*y/ly
        rng = np.random.default_rng(seed)
        uv, eta = 0.05*rng.normal(size=(mesh.num_cells, 3, 2)), 0.2*rng.normal(size=(mesh.num_cells, 3))
        return mesh, bath, uv, eta, alpha
    else:
        mesh, bath, uv, eta = channel_case(nx=60, ny=40, seed=seed, amp_eta=0.3, amp_u=0.2)
    return mesh, bath, uv, eta, None


def _device(path, mesh, bath, alpha, baseline):
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    dev = Swe2dDevice(mesh, bath, DT)
    for opt in (_lib.OPT_FUSED_STAGES, _lib.OPT_FLOW):       # the handle's own rule unless forced below (not the environment)
        dev.set_option(opt, None)
    if alpha is not None:
        dev.set_wetting_and_drying(alpha)
    if baseline or path == 'stages':
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 0)
    elif path in ('pair', 'quad', 'coupled'):
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 1)
        assert dev.fused_pair_info()[0], path
    elif path == 'triple':
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3)
        assert dev.fused_step_info()[0] and dev.fused_triple_info()[0]      # tables built here, outside any capture
    elif path in ('flow', 'wd'):
        assert dev.flow_supported() > 0, path
    return dev


def _ops(rng, path, n_ops):
    kinds = ['advance', 'advance', 'timed', 'stages', 'fe', 'fe_cells', 'set_state', 'capture', 'capture']
    if path == 'coupled':
        kinds += ['coupled', 'coupled']
    ops = []
    for _ in range(n_ops):
        k = kinds[rng.integers(len(kinds))]
        if k in ('advance', 'timed'):
            ops.append((k, int(rng.choice([1, 2, 3, 5])), bool(rng.integers(2))))
        elif k == 'coupled':
            ops.append((k, int(rng.choice([1, 2, 3]))))
        elif k == 'capture':
            what = ['advance', 'stages'] + (['step_pair'] if path == 'triple' else [])
            ops.append((k, what[rng.integers(len(what))], int(rng.integers(1, 3))))
        elif k == 'fe':
            ops.append((k, int(rng.integers(1, 3))))
        else:
            ops.append((k,))
    return ops


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('path', ['stages', 'pair', 'triple', 'flow', 'quad', 'wd', 'coupled'])
def test_step_paths_keep_the_state_contract(hip_lib, ref_so, path, seed):
    import torch
    mesh, bath, uv, eta, alpha = _case(path, seed)
    kw = dict(use_wetting_and_drying=True, wd_mode='nodal', wetting_and_drying_alpha=alpha) if alpha is not None else {}
    orc = make_oracle(mesh, bath, **kw)
    rt = None
    if path == 'coupled':
        from oracle.ref_lib import RefTracer
        rt = RefTracer(make_ref(mesh, bath), cell_topo_vertices=mesh.topo_vertex[mesh.cells])
    model = Model(orc, wd=alpha is not None, tracer=rt)
    dev = _device(path, mesh, bath, alpha, baseline=False)
    base = _device(path, mesh, bath, alpha, baseline=True)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    rng = np.random.default_rng(100 + seed)
    n = mesh.num_cells
    k = mesh.cells.shape[1]
    amp_u, amp_e = (0.05, 0.2) if alpha is not None else (0.2, 0.3)
    tid = None
    if path == 'coupled':
        cxy = mesh.cell_xy()
        T0 = np.where(cxy[:, :, 0] < 40e3, 0.0, 30.0) + 0.0
        tid = dev.add_tracer()
        assert base.add_tracer() == tid
        dev.tracer_set_state(tid, T0)
        base.tracer_set_state(tid, T0)
        model.T = T0.copy()

    def both(fn):
        fn(dev)
        fn(base)

    def read(i):
        _check_read(dev, base, model, i, path)

    with torch.cuda.stream(s):
        both(lambda d: d.set_state(uv, eta))
        model.set_state(uv, eta)
        read(0); read(2)
        for op in _ops(rng, path, 16):
            if op[0] == 'advance':
                both(lambda d: d.advance(op[1]))
                for _ in range(op[1]):
                    model.step()
            elif op[0] == 'timed':
                both(lambda d: d.advance_timed(op[1], per_launch=op[2]))
                for _ in range(op[1]):
                    model.step()
            elif op[0] == 'coupled':
                both(lambda d: d.advance_coupled(op[1], tracer_only=False, use_limiter=True))
                for _ in range(op[1]):
                    model.coupled()
                got = dev.tracer_get_state(tid)
                assert rel_linf(got, model.T) < TOL_TRACER
                assert np.array_equal(got, base.tracer_get_state(tid))
            elif op[0] == 'stages':
                for i in range(3):
                    both(lambda d: d.solve_stage(i))
                    model.stage(i)
                    if i < 2:
                        read(i)
                    if i == 0:
                        read(2)                      # stage 0 leaves buffer A alone
            elif op[0] == 'fe':
                both(lambda d: d.advance_forward_euler(op[1]))
                for _ in range(op[1]):
                    model.forward_euler()
            elif op[0] == 'fe_cells':
                cuts = sorted(set([0, n] + [int(c) for c in rng.integers(1, n, size=2)]))
                for d in (dev, base):
                    for c0, c1 in zip(cuts[:-1], cuts[1:]):
                        d.forward_euler_cells(c0, c1)
                    d.swap_state_buffers()
                model.forward_euler()
            elif op[0] == 'set_state':
                uv = amp_u*rng.normal(size=(n, k, 2))
                eta = amp_e*rng.normal(size=(n, k))
                both(lambda d: d.set_state(uv, eta))
                model.set_state(uv, eta)
            elif op[0] == 'capture':
                what, replays = op[1], op[2]
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
                    if what == 'advance':
                        dev.advance(2)
                    elif what == 'stages':
                        for i in range(3):
                            dev.solve_stage(i)
                    else:
                        dev.solve_step_cells(n)
                        dev.solve_step_cells(n)
                for _ in range(replays):
                    g.replay()
                s.synchronize()
                dev.synchronize()
                del g
                steps = (1 if what == 'stages' else 2)*replays
                if what == 'stages':
                    for _ in range(replays):
                        for i in range(3):
                            base.solve_stage(i)
                else:
                    base.advance(steps)
                for _ in range(steps):
                    model.step()
                model.captured()
            read(int(rng.integers(3)))
        for i in range(3):
            read(i)
        if tid is not None:
            got = dev.tracer_get_state(tid)
            assert rel_linf(got, model.T) < TOL_TRACER and np.array_equal(got, base.tracer_get_state(tid))
    dev.set_stream(None)
    dev.close()
    base.close()


# ---- the defects one by one

def _stage_handle(mesh, bath, fused=0):
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    dev = Swe2dDevice(mesh, bath, DT)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, fused)
    return dev


def _refused(fn):
    from thetis_amd import _lib
    with pytest.raises(_lib.Swe2dError) as err:
        fn()
    assert err.value.code == _lib.ERR_UNSUPPORTED, str(err.value)
    return str(err.value)


@pytest.mark.parametrize('how', ['advance_forward_euler', 'forward_euler_cells'])
def test_forward_euler_leaves_no_stage_solution(hip_lib, how):
    """After a ForwardEuler step buffer B holds the state before the step (the pointers were swapped): it is no U(1)."""
    mesh, bath, uv, eta = channel_case(nx=30, ny=20, seed=4, amp_eta=0.3, amp_u=0.2)
    model = Model(make_oracle(mesh, bath))
    dev = _stage_handle(mesh, bath)
    dev.set_state(uv, eta)
    model.set_state(uv, eta)
    for i in range(3):                                       # every stage solution in memory first
        dev.solve_stage(i)
    model.step()
    assert rel_linf(dev.get_state(0)[1], model.read(0)[1]) < TOL
    if how == 'advance_forward_euler':
        dev.advance_forward_euler(1)
    else:
        dev.forward_euler_cells(0, mesh.num_cells//3)
        dev.forward_euler_cells(mesh.num_cells//3, mesh.num_cells)
        dev.swap_state_buffers()
    model.forward_euler()
    _refused(lambda: dev.get_state(0))
    _refused(lambda: dev.get_state(1))
    u, e = dev.get_state()
    assert rel_linf(u, model.u) < TOL and rel_linf(e, model.e) < TOL
    dev.close()


def _triple_on_stream(mesh, bath, uv, eta):
    import torch
    from thetis_amd import _lib
    dev = _stage_handle(mesh, bath, fused=3)
    assert dev.fused_step_info()[0]                          # tables built outside the captures
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev.set_state(uv, eta)
    return dev, s, _lib


def test_two_odd_captures_are_each_reported_and_undone(hip_lib):
    """Two captures with one swe2d_solve_step_cells each, no call outside a capture between them: the count is per capture (two
    odd ones, not one even sum) - the error is reported, the host swaps are undone and the state is the one set before."""
    import torch
    mesh, bath, uv, eta = channel_case(nx=60, ny=40, seed=5, amp_eta=0.3, amp_u=0.2)
    n = mesh.num_cells
    model = Model(make_oracle(mesh, bath))
    model.set_state(uv, eta)
    dev, s, _lib = _triple_on_stream(mesh, bath, uv, eta)
    with torch.cuda.stream(s):
        graphs = []
        for _ in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
                dev.solve_step_cells(n)
            graphs.append(g)
        msg = _refused(dev.synchronize)
        assert 'odd number' in msg and msg.split(': ', 1)[1].startswith('2 '), msg
        dev.synchronize()                                    # reported once
        u, e = dev.get_state()
        assert np.array_equal(u, uv) and np.array_equal(e, eta), 'not the state from before the captures'
        dev.advance(2)
        for _ in range(2):
            model.step()
        u, e = dev.get_state()
        assert rel_linf(u, model.u) < TOL and rel_linf(e, model.e) < TOL
    dev.set_stream(None)
    dev.close()


@pytest.mark.parametrize('first_call', ['synchronize', 'get_state', 'advance', 'set_state'])
def test_an_odd_capture_is_reported_once_and_leaves_the_state_before_it(hip_lib, first_call):
    """The first call outside the capture that touches the state reports it (and does nothing else); afterwards get_state()
    is the state from before the capture and steps continue from there, whatever that first call was."""
    import torch
    mesh, bath, uv, eta = channel_case(nx=60, ny=40, seed=6, amp_eta=0.3, amp_u=0.2)
    n = mesh.num_cells
    model = Model(make_oracle(mesh, bath))
    model.set_state(uv, eta)
    dev, s, _lib = _triple_on_stream(mesh, bath, uv, eta)
    base = _stage_handle(mesh, bath)
    base.set_state(uv, eta)
    with torch.cuda.stream(s):
        dev.advance(1)                                       # eager: the three-stage kernel, one swap outside the capture
        base.advance(1)
        model.step()
        before = dev.get_state()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            dev.solve_step_cells(n)
        calls = {'synchronize': dev.synchronize, 'get_state': dev.get_state, 'advance': lambda: dev.advance(1),
                 'set_state': lambda: dev.set_state(uv, eta)}
        assert 'odd number' in _refused(calls[first_call])
        u, e = dev.get_state()
        assert np.array_equal(u, before[0]) and np.array_equal(e, before[1]), 'the odd capture left the handle on the other buffer'
        dev.advance(2)
        base.advance(2)
        for _ in range(2):
            model.step()
        u, e = dev.get_state()
        ub, eb = base.get_state()
        assert rel_linf(u, model.u) < TOL and rel_linf(e, model.e) < TOL
        assert np.array_equal(u, ub) and np.array_equal(e, eb)
    dev.set_stream(None)
    dev.close()
    base.close()


def test_triple_tables_are_not_built_inside_a_capture(hip_lib):
    """A handle whose three-stage tables are not built, SWE2D_OPT_FUSED_STAGES = 3 switched on: inside a capture
    fused_step_info / fused_triple_info answer "not built" without allocating, the capture stays valid (advance keeps the
    fused pair) and its replay gives the model's steps, the bits of the stage launches; outside, the tables are built."""
    import torch
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = channel_case(nx=60, ny=40, seed=7, amp_eta=0.3, amp_u=0.2)
    model = Model(make_oracle(mesh, bath))
    model.set_state(uv, eta)
    dev = Swe2dDevice(mesh, bath, DT)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, None)
    assert not dev.fused_step_info()[0] and not dev.fused_triple_info()[0]     # the rule: not at 4800 cells (nothing built)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3)
    base = _stage_handle(mesh, bath)
    base.set_state(uv, eta)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev.set_state(uv, eta)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            info_step = dev.fused_step_info()
            info_triple = dev.fused_triple_info()
            dev.advance(2)
        assert not info_step[0] and not info_triple[0], (info_step, info_triple)
        g.replay()
        g.replay()
        s.synchronize()
        dev.synchronize()
        base.advance(4)
        for _ in range(4):
            model.step()
        u, e = dev.get_state()
        ub, eb = base.get_state()
        assert rel_linf(u, model.u) < TOL and rel_linf(e, model.e) < TOL
        assert np.array_equal(u, ub) and np.array_equal(e, eb)
        assert dev.fused_step_info()[0] and dev.fused_triple_info()[0]          # outside a capture: built now
        dev.advance(1)                                                            # ... and taken (one swap, eager)
        base.advance(1)
        u, e = dev.get_state()
        ub, eb = base.get_state()
        assert np.array_equal(u, ub) and np.array_equal(e, eb)
    dev.set_stream(None)
    dev.close()
    base.close()


class _Recording(object):
    """a handle whose fused_step_info answers are kept"""

    def __init__(self, dev):
        self._dev, self.infos = dev, []

    def fused_step_info(self):
        r = self._dev.fused_step_info()
        self.infos.append(r)
        return r

    def __getattr__(self, name):
        return getattr(self._dev, name)


def test_rank_cycle_captured_on_a_handle_without_triple_tables(hip_lib):
    """What DistributedSwe2d._cycle_before_exchange does inside its per-cycle capture, on a rank handle whose three-stage tables
    were never built and SWE2D_OPT_FUSED_STAGES = 3: fused_step_info answers "not built" inside the capture, the cycle goes by the
    fused pair + stage launches, and the replay gives the bits of the stage launches on the owned cells."""
    import torch
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    from thetis_amd.distributed import DistributedSwe2d
    from thetis_amd.partition import build_partition, strip_owner
    mesh, bath, uv, eta = channel_case(nx=60, ny=40, seed=8, amp_eta=0.3, amp_u=0.2)
    every = 2
    p = build_partition(mesh, strip_owner(mesh, 2, axis=0), 0, halo_depth=3*every)
    g_ids = p.local_to_global

    def rank_handle(fused):
        d = Swe2dDevice(p, np.asarray(bath)[p.vertex_global], DT, n_owned=p.n_owned, boundary_len=p.boundary_len,
                        ranges=p.reorder_ranges())
        d.set_option(_lib.OPT_FLOW, 0)
        d.set_option(_lib.OPT_FUSED_STAGES, fused)
        d.set_state(uv[g_ids], eta[g_ids])
        return d

    def cycle(d):
        rank = types.SimpleNamespace(dev=d, part=p, _on_gpu=True, split_last_stage=False, stages_per_step=3)
        DistributedSwe2d._cycle_before_exchange(rank, every, 0)

    base = rank_handle(0)
    cycle(base)
    ub, eb = base.get_state()
    dev = rank_handle(3)
    rec = _Recording(dev)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev.set_state(uv[g_ids], eta[g_ids])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            cycle(rec)
        assert rec.infos and not any(i[0] for i in rec.infos), rec.infos
        g.replay()
        s.synchronize()
        dev.synchronize()
        u, e = dev.get_state()
    no = p.n_owned
    assert np.array_equal(u[:no], ub[:no]) and np.array_equal(e[:no], eb[:no])
    dev.set_stream(None)
    dev.close()
    base.close()


def test_stage_solutions_of_a_captured_step_are_refused(hip_lib):
    """Stage launches recorded in a capture run nothing then, and the host does not see the replays: get_state(0) / (1) are
    refused before the replay and after it (include/swe2d.h, swe2d_get_stage_state) - never the buffers of an earlier step -,
    get_state() is the replayed step; the next eager step makes them readable again."""
    import torch
    mesh, bath, uv, eta = channel_case(nx=30, ny=20, seed=9, amp_eta=0.3, amp_u=0.2)
    model = Model(make_oracle(mesh, bath))
    model.set_state(uv, eta)
    dev = _stage_handle(mesh, bath)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        dev.set_state(uv, eta)
        for i in range(3):
            dev.solve_stage(i)
        model.step()
        assert rel_linf(dev.get_state(1)[0], model.read(1)[0]) < TOL
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            for i in range(3):
                dev.solve_stage(i)
        _refused(lambda: dev.get_state(0))
        _refused(lambda: dev.get_state(1))
        g.replay()
        s.synchronize()
        dev.synchronize()
        model.step()
        _refused(lambda: dev.get_state(0))
        _refused(lambda: dev.get_state(1))
        u, e = dev.get_state()
        assert rel_linf(u, model.u) < TOL and rel_linf(e, model.e) < TOL
        for i in range(3):
            dev.solve_stage(i)
        model.step()
        for i in range(3):
            u, e = dev.get_state(i)
            assert rel_linf(u, model.read(i)[0]) < TOL and rel_linf(e, model.read(i)[1]) < TOL
    dev.set_stream(None)
    dev.close()


def test_malformed_switches_warn_and_take_the_defaults(hip_lib, monkeypatch):
    """THETIS_AMD_TRIPLE_TILE / THETIS_AMD_P2P_ZONE with a value that does not parse: a warning, and the handle is built as
    without them (the 11 x 8 patches of a mesh beyond the dataflow kernel; the library's own landing-zone rule)."""
    from thetis_amd import _lib
    from thetis_amd.device import Swe2dDevice
    from thetis_amd.mesh import RectangleMesh
    mesh = RectangleMesh(300, 220, 300e3, 220e3)              # 132 000 triangles: the patches are cut by themselves
    bath = np.full(len(mesh.vertex_xy), 20.0)
    for v in ('THETIS_AMD_TRIPLE_TILE', 'THETIS_AMD_P2P_ZONE', 'THETIS_AMD_FUSE12', 'THETIS_AMD_FLOW'):
        monkeypatch.delenv(v, raising=False)
    dev = Swe2dDevice(mesh, bath, DT)
    want = dev.fused_triple_info()
    dev.close()
    assert want[0]
    monkeypatch.setenv('THETIS_AMD_TRIPLE_TILE', '11x8')
    monkeypatch.setenv('THETIS_AMD_P2P_ZONE', 'nowhere')
    with pytest.warns(UserWarning) as rec:
        dev = Swe2dDevice(mesh, bath, DT)
    names = ' '.join(str(w.message) for w in rec)
    assert 'THETIS_AMD_TRIPLE_TILE' in names and 'THETIS_AMD_P2P_ZONE' in names, names
    assert dev.fused_triple_info() == want
    assert dev.get_option(_lib.OPT_P2P_ZONE) == -1
    dev.close()
