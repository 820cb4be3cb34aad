"""GPU: point probes (csrc/swe2d_probe.hip) give the bits of the host evaluation of get_state / tracer_get_state; Function.at samples
the device state without copying it; per-time-step detectors keep iterate() batched with the series of the step-by-step loop."""
import math
import os

import numpy as np
import pytest

from helpers import channel_case, quad_case
from thetis_amd.mesh import RectangleMesh
from thetis_amd.pointeval import PointLocator, evaluate

pytestmark = pytest.mark.gpu


def _points(mesh, n, seed):
    P = mesh.cell_xy()
    lo, hi = P.reshape(-1, 2).min(axis=0), P.reshape(-1, 2).max(axis=0)
    pts = np.random.default_rng(seed).uniform(lo + 1e-3*(hi - lo), hi - 1e-3*(hi - lo), size=(n, 2))
    loc = PointLocator(mesh, pts)
    keep = loc.cells >= 0
    return loc.cells[keep], loc.weights[keep]


def _probe_against_host(dev, cells, weights, tracer=None):
    fields = ['elev', 'uv'] + ([tracer] if tracer is not None else [])
    pid = dev.probe_create(cells, weights, fields, capacity=2)
    got = dev.probe_eval(pid)
    uv, eta = dev.get_state()
    ref = [evaluate(eta, cells, weights)[:, None], evaluate(uv, cells, weights)]
    if tracer is not None:
        ref.append(evaluate(dev.tracer_get_state(tracer), cells, weights)[:, None])
    assert np.array_equal(got, np.hstack(ref))
    dev.probe_append(pid)
    dev.probe_append(pid)
    with pytest.raises(Exception):                          # full: nothing written
        dev.probe_append(pid)
    rows = dev.probe_read(pid)
    assert rows.shape == (2,) + got.shape and np.array_equal(rows[1], got)
    assert dev.probe_read(pid).shape[0] == 0
    dev.probe_destroy(pid)


def test_probe_triangles(hip_lib):
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = channel_case(40, 12)
    dev = Swe2dDevice(mesh, bath, 5.0)
    dev.set_state(uv, eta)
    dev.advance(3)
    cells, w = _points(mesh, 300, 1)
    _probe_against_host(dev, cells, w)
    dev.close()


@pytest.mark.parametrize('kind', ['parallelogram', 'general'])
def test_probe_quadrilaterals(hip_lib, kind):
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = quad_case(skew=0.3) if kind == 'parallelogram' else quad_case(warp=0.3)
    dev = Swe2dDevice(mesh, bath, 5.0)
    dev.set_state(uv, eta)
    dev.advance(2)
    cells, w = _points(mesh, 200, 2)
    _probe_against_host(dev, cells, w)
    dev.close()


def test_probe_wetting_drying_and_tracer(hip_lib):
    """a Balzano-like beach (the elevation planes hold the displaced depth) and a tracer"""
    from thetis_amd.device import Swe2dDevice
    lx = 13800.0
    mesh = RectangleMesh(24, 3, lx, 7200.0)
    x = mesh.vertex_xy[:, 0]
    bath = x/lx*5.0 - 0.5
    dev = Swe2dDevice(mesh, bath, 10.0)
    dev.set_wetting_and_drying(0.5)
    n = mesh.num_cells
    X = mesh.cell_xy()[:, :, 0]
    dev.set_state(np.zeros((n, 3, 2)), np.maximum(0.3 - 0.0*X, -(X/lx*5.0 - 0.5)))
    tid = dev.add_tracer()
    dev.tracer_set_state(tid, np.exp(-((X - 5e3)/2e3)**2))
    dev.advance(4)
    cells, w = _points(mesh, 200, 3)
    _probe_against_host(dev, cells, w, tracer=tid)
    dev.close()


def _standing_wave(tmp_path, nx=20, n_steps_per_period=400, end_periods=1.0):
    from thetis_amd import DetectorsCallback, Function, get_functionspace, select_and_move_detectors, solver2d
    lx, ly = 5e3, 1e3
    mesh2d = RectangleMesh(nx, 1, lx, ly)
    depth = 100.0
    c = math.sqrt(9.81*depth)
    period = 2*lx/c
    dt = period/n_steps_per_period
    bath = Function(get_functionspace(mesh2d, 'CG', 1)).assign(depth)
    s = solver2d.FlowSolver2d(mesh2d, bath)
    s.options.timestep = dt
    s.options.simulation_export_time = dt
    s.options.simulation_end_time = end_periods*period - 0.1*dt
    s.options.no_exports = True
    s.options.swe_timestepper_type = 'SSPRK33'
    s.options.swe_timestepper_options.use_automatic_timestep = False
    s.options.output_directory = str(tmp_path)
    s.create_equations()
    s.assign_initial_conditions(elev=Function(get_functionspace(mesh2d, 'CG', 1)).interpolate(lambda x, y: np.cos(np.pi*x/lx)))
    xy = [[-2*lx, ly/2.], [-lx/2, ly/2.], [lx/4., ly/2.], [3*lx/4., ly/2.]]
    xy = select_and_move_detectors(mesh2d, xy, maximum_distance=lx)
    assert len(xy) == 3
    cb1 = DetectorsCallback(s, xy, ['elev_2d', 'uv_2d'], name='set1', append_to_log=True)
    cb2 = DetectorsCallback(s, xy[::-1], ['elev_2d'], name='set2', detector_names=['two', 'one', 'zero'], append_to_log=True)
    s.add_callback(cb1)
    s.add_callback(cb2)
    s.iterate()
    return s, lx, period, dt, n_steps_per_period


def test_standing_wave(hip_lib, tmp_path):
    """test/swe2d/test_standing_wave.py of the reference on SSPRK33 (a stable time step)"""
    s, lx, period, dt, n = _standing_wave(tmp_path)
    with np.load(os.path.join(str(tmp_path), 'diagnostic_set1.npz')) as df:
        assert list(df['field_dims']) == [1, 2]
        trange = np.arange(n + 1)*dt
        np.testing.assert_almost_equal(df['time'][:, 0], trange)
        np.testing.assert_allclose(df['detector1'][:, 0], np.cos(np.pi*(lx/4.)/lx)*np.cos(2*np.pi*trange/period), atol=5e-2, rtol=0.5)
    with np.load(os.path.join(str(tmp_path), 'diagnostic_set2.npz')) as df:
        assert list(df['field_dims']) == [1]
        np.testing.assert_allclose(df['one'][:, 0], np.cos(np.pi*(lx/4.)/lx)*np.cos(2*np.pi*trange/period), atol=5e-2, rtol=0.5)


def test_function_at_does_not_pull_the_state(hip_lib, tmp_path, monkeypatch):
    s, lx, period, dt, n = _standing_wave(tmp_path, end_periods=0.3)
    xy = [(lx/4 + 3.0, 500.0), (0.7*lx, 250.0)]
    stepper = s.timestepper
    loc = PointLocator(s.mesh2d, xy)

    def refuse(*a, **k):
        raise AssertionError('Function.at must not copy the state to the host')
    monkeypatch.setattr(stepper.device, 'get_state', refuse)
    got_e = s.fields.elev_2d.at(xy)
    got_u = s.fields.uv_2d.at(xy[0])
    monkeypatch.undo()
    uv, eta = stepper.device.get_state()
    assert np.array_equal(got_e, evaluate(eta, loc.cells, loc.weights))
    assert np.array_equal(got_u, evaluate(uv, loc.cells, loc.weights)[0])
    assert s.fields.elev_2d.at((-1.0, 1.0), dont_raise=True) is None


def _run_channel(tmp_path, mesh, bath, uv, eta, batched, dt, n_export, end_steps, sources=False):
    from thetis_amd import DetectorsCallback, Function, FunctionSpace, solver2d
    from thetis_amd.rungekutta import SSPRK33
    calls = []
    orig = SSPRK33.advance_steps

    def counting(self, t, n, probes=None):
        calls.append(n)
        return orig(self, t, n, probes=probes)
    SSPRK33.advance_steps = counting
    try:
        P1 = FunctionSpace(mesh, 'CG', 1)
        s = solver2d.FlowSolver2d(mesh, Function(P1).assign(bath))
        o = s.options
        o.timestep = dt
        o.simulation_export_time = n_export*dt
        o.simulation_end_time = (end_steps - 0.5)*dt
        o.no_exports = True
        o.swe_timestepper_type = 'SSPRK33'
        o.swe_timestepper_options.use_automatic_timestep = False
        o.output_directory = str(tmp_path)
        if sources:
            o.coriolis_frequency = 1e-4
            o.manning_drag_coefficient = 0.02
        s.create_equations()
        P = mesh.cell_xy()
        lo, hi = P.reshape(-1, 2).min(axis=0), P.reshape(-1, 2).max(axis=0)
        xy = np.random.default_rng(9).uniform(lo + 0.05*(hi - lo), hi - 0.05*(hi - lo), size=(100, 2))
        s.add_callback(DetectorsCallback(s, xy, ['elev_2d', 'uv_2d'], 'gauges'), 'timestep')
        ufs = FunctionSpace(mesh, 'DG', 1, vector=True)
        efs = FunctionSpace(mesh, 'DG', 1)
        s.assign_initial_conditions(elev=Function(efs).assign(eta.reshape(-1)), uv=Function(ufs).assign(uv.reshape(-1, 2)))
        if batched:
            s.iterate()
        else:
            for _ in s.create_iterator():
                pass
        cb = s.callbacks['timestep']['gauges']
        return [h[0] for h in cb.history], np.array([h[1] for h in cb.history]), calls
    finally:
        SSPRK33.advance_steps = orig


@pytest.mark.parametrize('case', ['dataflow', 'triple', 'sources', 'quads'])
def test_batched_equals_step_loop(hip_lib, tmp_path, case):
    dt = 10.0
    if case == 'triple':
        mesh, bath, uv, eta = channel_case(300, 250, amp_eta=0.05, amp_u=0.02)      # 150 k cells: the fused three-stage kernel
        n_export, end_steps, dt = 7, 21, 0.25
    elif case == 'quads':
        mesh, bath, uv, eta = quad_case(40, 20, amp_eta=0.05, amp_u=0.02)
        n_export, end_steps = 5, 15
    else:
        mesh, bath, uv, eta = channel_case(60, 20, amp_eta=0.05, amp_u=0.02)
        n_export, end_steps = 6, 18
    a_t, a_v, calls = _run_channel(tmp_path / 'a', mesh, bath, uv, eta, True, dt, n_export, end_steps, sources=(case == 'sources'))
    assert calls == [n_export]*(end_steps//n_export)                 # one advance_steps per export interval
    b_t, b_v, calls_b = _run_channel(tmp_path / 'b', mesh, bath, uv, eta, False, dt, n_export, end_steps, sources=(case == 'sources'))
    assert calls_b == []
    assert a_t == b_t and len(a_t) == end_steps
    assert np.array_equal(a_v, b_v)


@pytest.mark.parametrize('world', [2, 4])
def test_partitioned_detectors_equal_single_device(hip_lib, tmp_path, world):
    from detector_cases import assert_same, run_detectors
    single = run_detectors(1, str(tmp_path / 'one'), cpu=False)[0]
    for r in run_detectors(world, str(tmp_path / 'many'), cpu=False):
        assert_same(single, r)
