"""Statistics sets on the device (csrc/swe2d_stats.hip): the accumulators against a host replay of the same formulas bit for bit, on
every mesh kind, with wetting-drying and behind the buffer-swapping three-stage kernel; FlowSolver2d's batches with the callback
against the step-by-step loop; the merging of unsampled steps; the lifecycle of the sets.
"""
import numpy as np
import pytest

from helpers import channel_case
from stats_cases import (EPS, bathymetry, compare, empty_accumulators, omegas_for, random_state, replay_sample, stats_mesh,
                         weights_at)
from thetis_amd import DetectorsCallback, FieldStatisticsCallback, _lib
from thetis_amd.device import Swe2dDevice
from tide_cases import make_forcing, make_solver

pytestmark = pytest.mark.gpu
DT = 0.3
N_SAMPLES = 7
KS = (0, 2, 32)


def _sample_and_replay(dev, sets, n_samples=N_SAMPLES, t0=44714.1):
    """n_samples times: one step, one append to every set of ``sets`` ({K: id}), and the replay from ``get_state``"""
    want = {K: empty_accumulators((dev.n_cells, dev.npc), K) for K in sets}
    for j in range(n_samples):
        dev.advance(1)
        t = t0 + 300.0*j
        for K, sid in sets.items():
            dev.stats_append(sid, weights_at(omegas_for(K), t) if K else None)
        uv, eta = dev.get_state()
        assert np.isfinite(eta).all()
        for K in sets:
            replay_sample(want[K], uv, eta, weights_at(omegas_for(K), t))
    return want


@pytest.mark.parametrize('kind,wd', [('triangles', False), ('quads', False), ('general', False), ('triangles', True)])
def test_device_equals_host_replay(hip_lib, kind, wd):
    mesh = stats_mesh(kind)
    dev = Swe2dDevice(mesh, bathymetry(mesh, dry=wd), DT, boundary_len=mesh.boundary_len)
    assert dev.perm is not None and not np.array_equal(dev.perm, np.arange(mesh.num_cells))      # the read-back is permuted
    if wd:
        dev.set_wetting_and_drying(0.5)
    dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    dev.set_bc(1, {'elev': 0.2})
    dev.set_bc(2, {'un': 0.01})
    dev.set_state(*random_state(mesh))
    sets = {K: dev.stats_create(K) for K in KS}
    want = _sample_and_replay(dev, sets)
    for K, sid in sets.items():
        got, n = dev.stats_read(sid)
        assert n == N_SAMPLES and got.shape == (8 + 2*K, mesh.num_cells, mesh.cells.shape[1])
        worst = compare(got, want[K], n, '{:} wd={:} K={:d}'.format(kind, wd, K))
        print('{:} wd = {:} K = {:d}: s_sum / s3_sum max |device - host| = {:.2f} eps host (bound {:d})'.format(kind, wd, K, worst, n + 3))
        assert got[1].max() > got[0].min() and got[2].max() > 0.0
    dev.close()


def test_append_after_the_three_stage_kernel_reads_the_step_result(hip_lib):
    """the handle forced onto swe_fuse123_kernel (as tests/test_gpu_fuse3_rotation.py forces it): every step swaps the state buffers,
    the append that follows reads the buffer the step landed in"""
    mesh, bath, uv, eta = channel_case(nx=20, ny=13, lx=100e3, ly=50e3, seed=21, amp_eta=0.3, amp_u=0.2)
    assert mesh.num_cells == 520
    dev = Swe2dDevice(mesh, bath, 0.5)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, 3)
    dev.set_state(uv, eta)
    on, tiles, ring1, ring2 = dev.fused_triple_info()
    assert on and tiles > 0 and ring1 > 0 and ring2 > 0, (on, tiles, ring1, ring2)
    sets = {2: dev.stats_create(2)}
    want = _sample_and_replay(dev, sets)
    got, n = dev.stats_read(sets[2])
    assert n == N_SAMPLES
    worst = compare(got, want[2], n, 'three-stage kernel')
    print('three-stage kernel: s_sum / s3_sum max |device - host| = {:.2f} eps host'.format(worst))
    assert np.abs(got[3]/n - eta).max() > 0.0                # the state moved
    dev.close()


# ---- FlowSolver2d: batches
N_STEPS, EVERY = 24, 4


def _solver_run(mode, with_stats=True, with_detectors=False):
    """24 steps on the 520 triangles with a tide on the device at marker 1; mode 'iterate' | 'loop'.  Returns
    (accumulators, samples, uv, elev, detector history, advance calls)"""
    mesh = stats_mesh('triangles')
    forcing = make_forcing(mesh, K=3)
    s = make_solver(mesh, forcing, dt=DT, n_steps=N_STEPS, n_export=12)
    cb = det = None
    if with_stats:
        cb = FieldStatisticsCallback(s, harmonics=forcing, every=EVERY, export_to_hdf5=False)
        s.add_callback(cb, eval_interval='timestep')
    if with_detectors:
        det = DetectorsCallback(s, [(900.0, 700.0), (5100.0, 3300.0)], ['elev_2d', 'uv_2d'], 'gauges', export_to_hdf5=False)
        s.add_callback(det, eval_interval='timestep')
    dev = s.timestepper.device
    calls = []
    inner = dev.advance
    dev.advance = lambda n=1: (calls.append(int(n)), inner(n))[1]
    if mode == 'iterate':
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == N_STEPS
    acc, n = cb.accumulators() if cb is not None else (None, 0)
    hist = None if det is None else (np.array([h[0] for h in det.history]), np.array([h[1] for h in det.history]))
    out = (acc, n, s.fields.uv_2d.dat.data_ro.copy(), s.fields.elev_2d.dat.data_ro.copy(), hist, calls)
    dev.close()
    return out


@pytest.fixture(scope='module')
def batched(hip_lib):
    return _solver_run('iterate')


def test_batched_equals_step_by_step(hip_lib, batched):
    acc_b, n_b, uv_b, e_b, _, _ = batched
    acc_l, n_l, uv_l, e_l, _, calls_l = _solver_run('loop')
    assert n_b == n_l == N_STEPS//EVERY and calls_l == [1]*N_STEPS
    assert np.array_equal(acc_b, acc_l)
    assert acc_b.shape[0] == 8 + 2*3 and np.abs(acc_b[8:]).max() > 0.0
    _, _, uv_0, e_0, _, calls_0 = _solver_run('iterate', with_stats=False)
    assert calls_0 == [12, 12]
    for a, b in ((uv_b, uv_0), (e_b, e_0), (uv_l, uv_0), (e_l, e_0)):
        assert np.array_equal(a, b)
    assert np.abs(e_0).max() > 0.0


def test_detectors_and_statistics_side_by_side(hip_lib, batched):
    acc_d, n_d, uv_d, e_d, hist_d, calls_d = _solver_run('iterate', with_detectors=True)
    _, _, uv_0, e_0, hist_0, calls_0 = _solver_run('iterate', with_stats=False, with_detectors=True)
    assert calls_d == calls_0 == [1]*N_STEPS                  # a row per step: a call per step
    assert hist_d[0].shape == (N_STEPS,) and np.array_equal(hist_d[0], hist_0[0]) and np.array_equal(hist_d[1], hist_0[1])
    assert n_d == batched[1] and np.array_equal(acc_d, batched[0])
    assert np.array_equal(uv_d, uv_0) and np.array_equal(e_d, e_0) and np.array_equal(e_d, batched[3])


def test_unsampled_steps_are_merged(hip_lib, batched):
    """every = 4, no other consumer: 24 steps in two batches of 12 reach the device as 6 advance calls of 4 steps"""
    assert batched[5] == [4]*6


# ---- lifecycle
def _small_device():
    mesh = stats_mesh('triangles')
    dev = Swe2dDevice(mesh, bathymetry(mesh), DT, boundary_len=mesh.boundary_len)
    dev.set_state(*random_state(mesh))
    return mesh, dev


def test_lifecycle(hip_lib):
    mesh, dev = _small_device()
    shape = (mesh.num_cells, 3)
    a, b = dev.stats_create(2), dev.stats_create(0)
    assert (a, b) == (0, 1)
    acc, n = dev.stats_read(a)
    assert n == 0 and np.array_equal(acc, empty_accumulators(shape, 2))
    w = weights_at(omegas_for(2), 1234.5)
    dev.advance(1)
    dev.stats_append(a, w)
    one, n1 = dev.stats_read(a)
    again, n2 = dev.stats_read(a)                             # read does not clear
    assert n1 == n2 == 1 and np.array_equal(one, again) and not np.array_equal(one, acc)
    untouched, nb = dev.stats_read(b)                         # two sets on one handle do not disturb each other
    assert nb == 0 and np.array_equal(untouched, empty_accumulators(shape, 0))
    dev.stats_append(b)
    dev.stats_append(b)
    two, nb = dev.stats_read(b)
    assert nb == 2 and np.array_equal(two[3], one[3] + one[3]) and np.array_equal(dev.stats_read(a)[0], one)
    dev.stats_reset(a)                                        # reset restores the initial accumulators
    acc, n = dev.stats_read(a)
    assert n == 0 and np.array_equal(acc, empty_accumulators(shape, 2))
    assert dev.stats_read(b)[1] == 2
    dev.stats_destroy(a)                                      # a destroyed id is refused ...
    for call in (lambda: dev.stats_append(a, w), lambda: dev.stats_read(a), lambda: dev.stats_reset(a), lambda: dev.stats_destroy(a)):
        with pytest.raises(_lib.Swe2dError) as err:
            call()
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT
    assert dev.stats_create(32) == a                          # ... and reused
    assert dev.stats_read(a)[0].shape == (8 + 64,) + shape
    for K in (33, -1):
        with pytest.raises(_lib.Swe2dError) as err:
            dev.stats_create(K)
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(_lib.Swe2dError):                      # a set with constituents needs its weights
        dev._ck(dev.lib.swe2d_stats_append(dev.h, a, None))
    dev.close()


def test_refused_inside_a_stream_capture(hip_lib):
    import torch
    mesh, dev = _small_device()
    sid = dev.stats_create(1)
    w = weights_at(omegas_for(1), 10.0)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        buf = torch.zeros(16, device='cuda')
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            buf.add_(1.0)                                     # (the capture records something; nothing is replayed)
            for call in (lambda: dev.stats_append(sid, w), lambda: dev.stats_create(0), lambda: dev.stats_read(sid),
                         lambda: dev.stats_reset(sid), lambda: dev.stats_destroy(sid)):
                with pytest.raises(_lib.Swe2dError) as err:
                    call()
                assert err.value.code == _lib.ERR_UNSUPPORTED
        s.synchronize()
        dev.advance(1)                                        # the handle is usable, the set untouched
        dev.stats_append(sid, w)
        acc, n = dev.stats_read(sid)
    dev.set_stream(None)
    uv, eta = dev.get_state()
    want = replay_sample(empty_accumulators(eta.shape, 1), uv, eta, w)
    assert n == 1
    compare(acc, want, 1, 'after the capture')
    dev.close()
