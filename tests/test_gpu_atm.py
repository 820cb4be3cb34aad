"""The atmospheric record on the device (csrc/swe2d_atm.hip): evaluation against the host expression, what the launches leave alone,
the batched advance against the step-by-step path bit for bit and against the host-forced path, what the step plan reports and
refuses, and FlowSolver2d's batches."""
import numpy as np
import pytest

from atm_cases import (EPS, METHODS, atm_mesh, eval_times, make_atm, make_solver, run_atm_ranks, stress_sensitivity, _atm_case)
from helpers import rel_linf
from thetis_amd import _lib
from thetis_amd.device import Swe2dDevice, TideValues
from tide_cases import LX, LY, make_forcing

pytestmark = pytest.mark.gpu
DT = 0.3
TOL_FORCED = 1e-10              # the suite's bound for time-dependent forcing data (tests/test_gpu_tide.py)
T_BASE, K_FIRST, C = 0.7, 3, (0.0, 1.0, 0.5)


def _bath(mesh):
    x, y = mesh.vertex_xy.T
    return 12.0 - 3.0*x/LX + 0.5*np.sin(y/900.0)


def _state(mesh, seed=3):
    rng = np.random.default_rng(seed)
    n, k = mesh.cells.shape
    uv = 0.05*rng.normal(size=(n, k, 2))
    eta = 0.1*np.cos(np.pi*mesh.cell_xy()[:, :, 0]/LX) + 0.01*rng.normal(size=(n, k))
    return uv, eta


def _stage_times(n, forward_euler=False):
    out = []
    for k in range(n):
        t_k = T_BASE + (K_FIRST + k)*DT
        out += [t_k + DT] if forward_euler else [t_k + c*DT for c in C]
    return out


def _device(kind='triangles', wind=True, pressure=True, method='LargeYeager2009', n_t=5, wd=False, with_atm=True, tide=False,
            check_times=None):
    """a handle on a closed basin (marker 2: a constant normal velocity) with the record of ``make_atm``"""
    mesh = atm_mesh(kind)
    dev = Swe2dDevice(mesh, _bath(mesh) - (11.5 if wd else 0.0), DT, boundary_len=mesh.boundary_len)
    f = make_atm(mesh, n_t=n_t, method=method, wind=wind, pressure=pressure, check_times=check_times)
    if wd:
        dev.set_wetting_and_drying(0.5)
    dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    if with_atm:
        dev.atm_set(f.times, f.wind_u, f.wind_v, f.pressure, method=method)
    if tide:
        g = make_forcing(mesh, K=3)
        dev.tide_set([dev._slot(1)], g.omegas, *g.facet_tables(dev, 1))
        dev.set_bc(1, {'elev': TideValues()})
    dev.set_bc(2, {'un': 0.01})
    return mesh, dev, f


def _host_nodal(mesh, f, t):
    """what ``set_fields(t)`` gives at the DG nodes: (wind stress (N, k, 2) or None, pressure (N, k) or None)"""
    f.set_fields(t)
    w = None if f.wind_stress_field is None else f.wind_stress_field.dat.data_ro[mesh.cells]
    p = None if f.atm_pressure_field is None else f.atm_pressure_field.dat.data_ro[mesh.cells]
    return w, p


def _stress_bound(f, t, want):
    """(S + 1) eps |tau_c| per component: see test_evaluation_matches_set_fields"""
    j, al = f.bracket(t)
    u, v = (1.0 - al)*f.wind_u[j] + al*f.wind_u[j + 1], (1.0 - al)*f.wind_v[j] + al*f.wind_v[j + 1]
    S = stress_sensitivity(f.method, np.concatenate([np.linspace(1e-3, 45.0, 20001), np.sqrt(u*u + v*v)]))
    assert 0.0 < S < 20.0
    return S, (S + 1.0)*EPS*np.abs(want)


# ---- 1. evaluation

@pytest.mark.parametrize('kind,n_t', [('triangles', 5), ('triangles', 2), ('quads', 5), ('general', 5), ('tri280', 5), ('tri280', 2)])
@pytest.mark.parametrize('method', METHODS)
def test_evaluation_matches_set_fields(hip_lib, method, kind, n_t):
    """The pressure is bit-equal.  |device - host| <= (S + 1) eps |tau_c| per stress component tau_c, with S evaluated below.

    Both sides evaluate, with no fused operation (contraction off on the device, numpy on the host),
        x = fl(fl((1 - alpha)*x_j) + fl(alpha*x_{j+1}))  for u, v, p;   m = sqrt_x(fl(fl(u*u) + fl(v*v)));
        tau = fl(fl(C_D(m)*rho_air)*m);   tau_c = fl(tau*c),  c = u, v
    on identical inputs: j and alpha come from the same IEEE expression on the host of either side, and `+ - * /` are correctly
    rounded on both, so the pressure has the same bits and so has everything that enters the square root.  The two square roots are
    each within one ulp of the true root's rounding, so the device's m is the host's or one of its two neighbours m'.  From m on,
    tau is again the same correctly rounded function on both sides: the device's tau is tau(m) or tau(m'), and
    S = max |tau(m') - tau(m)|/(eps |tau(m)|) - how many eps one ulp of the speed moves C_D(m)*rho_air*m by, its log-sensitivity
    1 + m C_D'/C_D times the rounding of the operations behind it - is evaluated numerically on the CPU (atm_cases.stress_sensitivity)
    over 0 .. 45 m/s and over the record's own speeds.  The last product adds one rounding of its own: 'the 1'.  Zero wind: m = 0
    exactly on both sides, the bound is 0.  No speed is within 1e-6 of a switch of C_D (asserted by make_atm), so both sides take the
    same branch.  If the device's square root rounds as numpy's, the difference is 0."""
    mesh, dev, f = _device(kind, method=method, n_t=n_t)              # (n_t = 2: the bracket is clamped to j = 0 at every time)
    worst = 0.0
    for t in eval_times(f.times):
        dev.atm_eval(t)
        gw, gp = dev.atm_read()
        ww, wp = _host_nodal(mesh, f, t)
        S, bound = _stress_bound(f, t, ww)
        assert gp.shape == wp.shape and np.array_equal(gp, wp)
        err = np.abs(gw - ww)
        worst = max(worst, float(err.max()))
        print('{:} {:} t = {:g}: S = {:.2f}, max |device - host| stress = {:.3e} (max |tau| {:.3f})'.format(
            kind, method, t, S, err.max(), np.abs(ww).max()))
        assert gw.shape == ww.shape and np.isfinite(gw).all()
        assert (err <= bound).all()
        assert np.abs(ww).max() > 1.0 and (ww == 0.0).any()
    print('{:} {:}: measured maximum over the times {:.3e}'.format(kind, method, worst))
    dev.close()


# ---- 2. untouched data
@pytest.mark.parametrize('kind', ['triangles', 'tri280', 'quads'])
def test_fields_outside_the_record_keep_their_bits(hip_lib, kind):
    """the planes of a field whose bit is clear keep an uploaded field bit for bit, and Coriolis and a drag field are what they were:
    a handle that went through evaluations and ``atm_clear`` has the tendency and the steps of one that got the same planes by
    ``set_field``.  (That a handle on which ``atm_set`` was never called steps as before this kernel existed is what the existing suite
    checks against its oracle - tests/test_gpu_fuzz.py::test_random_option_combinations_match_oracle and the golden states of
    tests/test_gpu_solver2d.py -, and tests/test_gpu_tide.py for a handle with a tide alone.)"""
    rng = np.random.default_rng(11)
    for wind in (True, False):
        mesh, dev, f = _device(kind, wind=wind, pressure=not wind)
        n, k = mesh.cells.shape
        mine_w, mine_p = rng.normal(size=(n, k, 2)), 1e5 + rng.normal(size=(n, k))
        cor, drag = 1e-4*(1.0 + rng.uniform(size=(n, k))), 0.02 + 0.01*rng.uniform(size=(n, k))
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, None)
        dev.set_field(_lib.FIELD_CORIOLIS, cor)
        dev.set_field(_lib.FIELD_MANNING_DRAG, drag)
        if wind:
            dev.set_field(_lib.FIELD_ATMOSPHERIC_PRESSURE, mine_p)
        else:
            dev.set_field(_lib.FIELD_WIND_STRESS, mine_w)
        for t in eval_times(f.times):
            dev.atm_eval(t)
        gw, gp = dev.atm_read()
        ww, wp = _host_nodal(mesh, f, eval_times(f.times)[-1])
        if wind:
            assert np.array_equal(gp, mine_p) and (np.abs(gw - ww) <= _stress_bound(f, eval_times(f.times)[-1], ww)[1]).all()
        else:
            assert np.array_equal(gw, mine_w) and np.array_equal(gp, wp)
        dev.atm_clear()
        assert all(np.array_equal(a, b) for a, b in zip(dev.atm_read(), (gw, gp)))        # the planes keep their last values
        twin = Swe2dDevice(mesh, _bath(mesh), DT, boundary_len=mesh.boundary_len)
        twin.set_bc(2, {'un': 0.01})
        twin.set_field(_lib.FIELD_CORIOLIS, cor)
        twin.set_field(_lib.FIELD_MANNING_DRAG, drag)
        twin.set_field(_lib.FIELD_WIND_STRESS, gw)
        twin.set_field(_lib.FIELD_ATMOSPHERIC_PRESSURE, gp)
        uv, eta = _state(mesh)
        for d in (dev, twin):
            d.set_state(uv, eta)
        for a, b in zip(dev.tendency(), twin.tendency()):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        for d in (dev, twin):
            d.advance(2)
        for a, b in zip(dev.get_state(), twin.get_state()):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        dev.close()
        twin.close()


@pytest.mark.parametrize('freed', ['wind', 'pressure'])
def test_a_freed_field_leaves_the_other_right(hip_lib, freed):
    """a record with both quantities (three doubles per vertex), the planes of one field freed behind its back
    (``set_field(field, None)``): the launches write the other field alone, from its own column of the record - bit for bit what
    ``set_fields`` gives - and a step runs; a new ``atm_set`` brings the planes back"""
    mesh, dev, f = _device('tri280')
    dev.set_field(_lib.FIELD_WIND_STRESS if freed == 'wind' else _lib.FIELD_ATMOSPHERIC_PRESSURE, None)
    for t in eval_times(f.times):
        dev.atm_eval(t)
        gw, gp = dev.atm_read(wind=freed != 'wind', pressure=freed != 'pressure')
        ww, wp = _host_nodal(mesh, f, t)
        if freed == 'wind':
            assert gw is None and np.array_equal(gp, wp)
        else:
            assert gp is None and (np.abs(gw - ww) <= _stress_bound(f, t, ww)[1]).all() and np.abs(gw).max() > 1.0
    with pytest.raises(_lib.Swe2dError):
        dev.atm_read()                                                 # the freed planes are not there
    dev.set_state(*_state(mesh))
    dev.tide_clock(T_BASE, K_FIRST)
    dev.advance(2)
    assert all(np.isfinite(a).all() for a in dev.get_state())
    dev.atm_set(f.times, f.wind_u, f.wind_v, f.pressure)
    t = eval_times(f.times)[3]
    dev.atm_eval(t)
    gw, gp = dev.atm_read()
    ww, wp = _host_nodal(mesh, f, t)
    assert np.array_equal(gp, wp) and (np.abs(gw - ww) <= _stress_bound(f, t, ww)[1]).all()
    dev.close()


# ---- 3. batched = step by step, bit for bit
def _step_by_step(dev, n, forward_euler=False, tid=None, tide=False):
    for k in range(n):
        t_k = T_BASE + (K_FIRST + k)*DT
        if forward_euler:
            dev.atm_eval(t_k + DT)
            dev.forward_euler_cells(0, dev.n_cells)
            dev.swap_state_buffers()
            continue
        for i in range(3):
            if tide:
                dev.tide_eval(t_k + C[i]*DT)
            dev.atm_eval(t_k + C[i]*DT)
            dev.solve_stage(i)
        if tid is not None:
            for i in range(3):
                dev.tracer_solve_stage(tid, i)
            dev.tracer_limit(tid)


@pytest.mark.parametrize('case', ['triangles', 'quads', 'general', 'wetting_drying', 'forward_euler', 'tracer', 'tide'])
def test_batched_advance_equals_step_by_step(hip_lib, case):
    kind = case if case in ('triangles', 'quads', 'general') else 'triangles'
    fe = case == 'forward_euler'
    res = []
    for batched in (True, False):
        mesh, dev, f = _device(kind, wd=(case == 'wetting_drying'), tide=(case == 'tide'), check_times=_stage_times(5, fe))
        uv, eta = _state(mesh)
        tid = None
        if case == 'tracer':
            tid = dev.add_tracer()
            dev.tracer_set_state(tid, 1.0 + (mesh.cell_xy()[:, :, 0] > 0.5*LX))
        dev.set_state(uv, eta)
        if batched:
            dev.tide_clock(T_BASE, K_FIRST)
            if fe:
                dev.advance_forward_euler(5)
            elif case == 'tracer':
                dev.advance_coupled(5, use_limiter=True)
            else:
                dev.advance(2)
                dev.advance(3)                                         # the library counts the steps on
        else:
            _step_by_step(dev, 5, forward_euler=fe, tid=tid, tide=(case == 'tide'))
        res.append(dev.get_state() + dev.atm_read() + ((dev.tide_read(),) if case == 'tide' else ())
                   + ((dev.tracer_get_state(tid),) if tid is not None else ()))
        ww, wp = _host_nodal(mesh, f, _stage_times(5, fe)[-1])
        assert np.array_equal(res[-1][3], wp)                          # the last stage of the last step was evaluated at its time
        assert (np.abs(res[-1][2] - ww) <= _stress_bound(f, _stage_times(5, fe)[-1], ww)[1]).all()
        dev.close()
    for a, b in zip(*res):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert np.abs(res[0][1] - _state(atm_mesh(kind))[1]).max() > 1e-4   # (the steps moved the state)


# ---- 4. against the host-forced path
def test_batched_advance_against_host_forced_path(hip_lib):
    """20 steps of the batched run of (3) against the existing path: ``set_fields`` on the host at every stage time, the per-vertex
    upload of both fields (swe2d_set_field_vertex), one stage launch.  The tolerance is the suite's own for time-dependent forcing
    data (tests/test_gpu_tide.py, TOL_FORCED)."""
    mesh, dev, f = _device('triangles', check_times=_stage_times(20))
    uv, eta = _state(mesh)
    dev.set_state(uv, eta)
    dev.tide_clock(T_BASE, K_FIRST)
    dev.advance(20)
    ua, ea = dev.get_state()
    dev.close()
    mesh, host, f = _device('triangles', with_atm=False)
    host.set_state(uv, eta)
    for t, i in zip(_stage_times(20), list(range(3))*20):
        f.set_fields(t)
        host.set_field_vertex(_lib.FIELD_WIND_STRESS, f.wind_stress_field.dat.data_ro)
        host.set_field_vertex(_lib.FIELD_ATMOSPHERIC_PRESSURE, f.atm_pressure_field.dat.data_ro)
        host.solve_stage(i)
    ub, eb = host.get_state()
    host.close()
    print('device record against host-forced path after 20 steps: rel_linf eta {:.3e}, uv {:.3e}'.format(rel_linf(ea, eb), rel_linf(ua, ub)))
    assert rel_linf(ea, eb) < TOL_FORCED and rel_linf(ua, ub) < TOL_FORCED
    # ... and the forcing drove it: the same handle without it ends elsewhere
    mesh, rest, _ = _device('triangles', with_atm=False)
    rest.set_state(uv, eta)
    rest.advance(20)
    assert np.abs(rest.get_state()[1] - ea).max() > 1e-5
    rest.close()


# ---- 5. plan and refusals
def _plan(dev):
    return dev.fused_pair_info(), dev.fused_triple_info(), dev.fused_step_info(), dev.flow_supported()


@pytest.mark.parametrize('fused', [None, 3])
def test_plan_declines_a_record(hip_lib, fused):
    mesh, fresh, _ = _device('triangles', with_atm=False)
    mesh, dev, f = _device('triangles')
    for d in (fresh, dev):
        d.set_scalar(_lib.SCALAR_MANNING_DRAG, None)
        if fused is not None:
            d.set_option(_lib.OPT_FUSED_STAGES, fused)
            d.set_option(_lib.OPT_FLOW, 0)
    # the fresh handle gets the planes the record allocated, constant in time: what the plan is compared against after atm_clear
    dev.atm_eval(1.0)
    w, p = dev.atm_read()
    fresh.set_field(_lib.FIELD_WIND_STRESS, w)
    fresh.set_field(_lib.FIELD_ATMOSPHERIC_PRESSURE, p)
    want = _plan(fresh)
    assert want[3] == 1 and (fused is None or want[1][0])          # (1: the dataflow kernel with source terms)
    got = _plan(dev)
    assert not got[0][0] and not got[1][0] and not got[2][0] and got[3] == 0
    for call in (lambda: dev.solve_flow([mesh.num_cells]*3), lambda: dev.solve_step_cells(mesh.num_cells),
                 lambda: dev.solve_stage_pair_cells(mesh.num_cells, mesh.num_cells), lambda: dev.advance_timed(1, per_launch=True)):
        with pytest.raises(_lib.Swe2dError) as err:
            call()
        assert err.value.code == _lib.ERR_UNSUPPORTED
    dev.atm_clear()
    assert _plan(dev) == want                                          # the handle has its step kernels back
    fresh.close()
    dev.close()


def test_advance_past_the_record_fails_and_touches_nothing(hip_lib):
    for fe in (False, True):
        mesh, dev, f = _device('triangles')
        uv, eta = _state(mesh)
        dev.set_state(uv, eta)
        dev.tide_clock(0.0, 0)
        dev.advance(2)
        before = dev.get_state() + dev.atm_read()
        # the record ends at 9.5: step 31 of the clock starts at 9.3, its last stages leave it
        dev.tide_clock(0.0, 29)
        with pytest.raises(_lib.Swe2dError) as err:
            (dev.advance_forward_euler if fe else dev.advance)(3)
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT and '9.5' in str(err.value) and 'outside' in str(err.value)
        for a, b in zip(before, dev.get_state() + dev.atm_read()):
            assert np.array_equal(a, b)
        # the clock was left alone: the two steps that fit give what a fresh count from 29 gives
        (dev.advance_forward_euler if fe else dev.advance)(2)
        ua, ea = dev.get_state()
        dev.set_state(*before[:2])
        dev.tide_clock(0.0, 29)
        (dev.advance_forward_euler if fe else dev.advance)(2)
        ub, eb = dev.get_state()
        assert np.isfinite(ea).all() and np.array_equal(ea, eb) and np.array_equal(ua, ub)
        with pytest.raises(_lib.Swe2dError) as err:
            dev.atm_eval(9.6)
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT
        dev.close()


def test_atm_set_validates(hip_lib):
    mesh, dev, f = _device('triangles', with_atm=False)
    bad_times = f.times.copy()
    bad_times[2] = bad_times[1]
    nan_p = f.pressure.copy()
    nan_p[1, 3] = np.nan
    for kw in (dict(times=bad_times), dict(pressure=nan_p), dict(times=f.times[:1], wind_u=f.wind_u[:1], wind_v=f.wind_v[:1],
                                                                  pressure=f.pressure[:1])):
        args = dict(times=f.times, wind_u=f.wind_u, wind_v=f.wind_v, pressure=f.pressure)
        args.update(kw)
        with pytest.raises(_lib.Swe2dError) as err:
            dev.atm_set(args['times'], args['wind_u'], args['wind_v'], args['pressure'])
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        dev.atm_set(f.times, f.wind_u[:, :-1], f.wind_v[:, :-1], None)
    with pytest.raises(_lib.Swe2dError):
        dev.atm_eval(1.0)                                              # no record
    assert _plan(dev)[3] > 0
    dev.close()


def test_calls_inside_a_capture_are_refused(hip_lib):
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
            for call in (lambda: dev.advance(1), lambda: dev.advance_forward_euler(1), lambda: dev.atm_eval(1.0), dev.atm_read,
                         dev.atm_clear, lambda: dev.atm_set(f.times, f.wind_u, f.wind_v, f.pressure)):
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


# ---- 6. solver
def _solver_run(tmp_path, batched, detectors):
    from thetis_amd import DetectorsCallback
    mesh = atm_mesh('triangles')
    f = make_atm(mesh, n_t=5)
    s = make_solver(mesh, f, f, dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path))
    assert s.timestepper.wants_clock and not s.timestepper.forced_per_stage
    if detectors:
        s.add_callback(DetectorsCallback(s, [(0.3*LX, 0.4*LY), (0.8*LX, 0.7*LY)], ['elev_2d', 'uv_2d'], 'gauges'), 'timestep')
    dev = s.timestepper.device
    calls = []
    inner = dev.advance
    dev.advance = lambda n=1: (calls.append(int(n)), inner(n))[1]
    if batched:
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    hist = s.callbacks['timestep']['gauges'].history if detectors else []
    return (s.fields.elev_2d.dat.data_ro.copy(), s.fields.uv_2d.dat.data_ro.copy(), [h[0] for h in hist],
            np.array([h[1] for h in hist]), s.simulation_time, s.iteration, calls)


def test_iterate_batches_an_atmospherically_forced_run(hip_lib, tmp_path):
    a = _solver_run(tmp_path / 'a', True, False)
    assert a[6] == [4, 4]                                              # one device.advance per export interval
    b = _solver_run(tmp_path / 'b', False, False)
    assert b[6] == [1]*8
    assert a[4] == b[4] and a[5] == b[5] == 8
    for x, y in zip(a[:2], b[:2]):
        assert np.isfinite(x).all() and np.array_equal(x, y)
    # a per-step DetectorsCallback sees the same rows either way, and the state is the same again
    c = _solver_run(tmp_path / 'c', True, True)
    d = _solver_run(tmp_path / 'd', False, True)
    assert c[2] == d[2] and len(c[2]) == 8 and np.isfinite(c[3]).all() and np.array_equal(c[3], d[3])
    for x, y in zip(c[:2], a[:2]):
        assert np.array_equal(x, y)
    # the forcing drove it: the basin without it ends elsewhere
    e = make_solver(atm_mesh('triangles'), None, None, dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path / 'e'))
    e.iterate()
    assert np.abs(e.fields.elev_2d.dat.data_ro - a[0]).max() > 1e-6


def test_record_is_uploaded_once_per_object(hip_lib, tmp_path):
    """the record goes up when the stepper is built, and again only for another object (or another set of quantities)"""
    mesh = atm_mesh('triangles')
    f = make_atm(mesh, n_t=5)
    s = make_solver(mesh, f, f, dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path))
    ts = s.timestepper
    calls = []
    inner = ts.device.atm_set
    ts.device.atm_set = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    s.iterate()
    ts._push_fields(only_changed=True)
    assert calls == []
    g = make_atm(mesh, n_t=2)
    ts.fields['wind_stress'] = ts.fields['atmospheric_pressure'] = g
    ts._push_fields(only_changed=True)
    ts._push_fields(only_changed=True)
    assert calls == [1] and ts._device_atm is g
    ts.fields['atmospheric_pressure'] = None                            # wind alone: another record layout
    ts._push_fields(only_changed=True)
    assert calls == [1, 1]
    ts.fields['wind_stress'] = None
    ts._push_fields(only_changed=True)
    assert ts._device_atm is None and not ts.wants_clock and calls == [1, 1]


def test_update_forcings_path_still_works(hip_lib, tmp_path):
    """the reference's way - the fields as option values, ``set_fields`` from ``update_forcings`` - against the object as option
    value, within the tolerance of (4)"""
    mesh = atm_mesh('triangles')
    f = make_atm(mesh, n_t=5)
    a = make_solver(mesh, f, f, dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path / 'a'))
    a.iterate()
    g = make_atm(mesh, n_t=5)
    b = make_solver(mesh, g.wind_stress_field, g.atm_pressure_field, dt=DT, n_steps=8, n_export=4, outdir=str(tmp_path / 'b'))
    b.iterate(update_forcings=g.set_fields)
    ea, eb = a.fields.elev_2d.dat.data_ro, b.fields.elev_2d.dat.data_ro
    print('object as option value against update_forcings: rel_linf eta {:.3e}'.format(rel_linf(ea, eb)))
    assert rel_linf(ea, eb) < TOL_FORCED and rel_linf(a.fields.uv_2d.dat.data_ro, b.fields.uv_2d.dat.data_ro) < TOL_FORCED


def test_two_ranks_take_the_host_path(hip_lib, tmp_path):
    """several ranks: every rank calls ``set_fields`` on the host per stage - the single-rank, device-evaluated state within the
    tolerance of (4), nothing raised"""
    single = _atm_case(str(tmp_path / 'one'))
    assert single.timestepper.wants_clock
    e1, u1 = single.fields.elev_2d.dat.data_ro.copy(), single.fields.uv_2d.dat.data_ro.copy()
    ranks = run_atm_ranks(2, str(tmp_path))
    for r in ranks:
        assert r['iteration'] == single.iteration == 20 and r['simulation_time'] == single.simulation_time
        print('two ranks against one: rel_linf eta {:.3e}, uv {:.3e}'.format(rel_linf(r['elev'], e1), rel_linf(r['uv'], u1)))
        assert rel_linf(r['elev'], e1) < TOL_FORCED and rel_linf(r['uv'], u1) < TOL_FORCED
