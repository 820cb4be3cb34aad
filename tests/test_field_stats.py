"""Field statistics on the host (thetis_amd/fieldstats.py): the known answer of the harmonic fit, its refusal of ill-conditioned
records, the sampling schedule through FlowSolver2d on the host stand-in device, and the ABI of the built library."""
import ctypes
import os
import types

import numpy as np
import pytest

from cpu_device import CpuSwe2dDevice
from stats_cases import K1, M2, S2, empty_accumulators, replay_sample, weights_at
from thetis_amd import Constant, FieldStatisticsCallback, _lib, callback, fieldstats, solver2d
from tide_cases import make_solver, tide_mesh


def _bare_callback(harmonics, **kw):
    """a callback without a solver behind it: fed through ``add_host_sample``"""
    solver = types.SimpleNamespace(comm=types.SimpleNamespace(size=1, rank=0), simulation_time=0.0, iteration=0)
    return FieldStatisticsCallback(solver, harmonics=harmonics, **kw)


def test_exported_from_the_package_and_from_callback():
    assert callback.FieldStatisticsCallback is fieldstats.FieldStatisticsCallback is FieldStatisticsCallback
    assert 'FieldStatisticsCallback' in callback.__all__


def test_known_answer_of_the_fit():
    """e(t) = m + sum_k A_k cos(omega_k t - phi_k) with M2, S2, K1, 600 samples 300 s apart (50 h: cond(W) = 82), 50 nodes with
    random m, A, phi: the fit returns them within 1e-9 relative - cond(W) times the n*eps of the plain sums is 5e-12.
    (m, A and phi are drawn away from zero, so that 'relative' has a scale: |m| >= 0.05, A >= 0.1, |phi| in [0.1, 3].)"""
    rng = np.random.default_rng(11)
    names, om = ['M2', 'S2', 'K1'], np.array([M2, S2, K1])
    n_nodes = 50
    m = rng.uniform(0.05, 1.0, n_nodes)*rng.choice([-1.0, 1.0], n_nodes)
    A = rng.uniform(0.1, 2.0, (3, n_nodes))
    phi = rng.uniform(0.1, 3.0, (3, n_nodes))*rng.choice([-1.0, 1.0], (3, n_nodes))
    cb = _bare_callback(dict(zip(names, om)))
    uv = np.zeros((n_nodes, 1, 2))
    for j in range(600):
        t = 300.0*(j + 1)
        e = m + sum(A[k]*np.cos(om[k]*t - phi[k]) for k in range(3))
        uv[:, 0, 0], uv[:, 0, 1] = 0.3*np.cos(M2*t), 0.4*np.cos(M2*t)
        cb.add_host_sample(t, uv, e.reshape(n_nodes, 1))
    assert np.linalg.cond(cb.W) < 100.0
    r = cb.result()
    assert cb.n_samples == 600
    rel = lambda got, want: float((np.abs(got - want)/np.abs(want)).max())
    worst = {'mean': rel(r['elev_fit_mean'], m)}
    for k, c in enumerate(names):
        worst['A_' + c] = rel(r['elev_amp'][c], A[k])
        worst['phi_' + c] = rel(r['elev_phase'][c], phi[k])
    print(worst)
    assert max(worst.values()) < 1e-9, worst
    # the other statistics of the same record: |u| = 0.5 |cos(M2 t)|
    c = np.abs(np.cos(M2*300.0*np.arange(1, 601)))
    assert np.allclose(r['speed_max'], 0.5*c.max(), rtol=1e-14) and np.allclose(r['speed_mean'], 0.5*c.mean(), rtol=1e-13)
    assert np.allclose(r['speed_cubed_mean'], 0.125*(c**3).mean(), rtol=1e-13)
    assert r['uv_mean'].shape == (n_nodes, 2) and r['elev_min'].shape == (n_nodes,)
    assert (r['elev_min'] <= r['elev_mean']).all() and (r['elev_mean'] <= r['elev_max']).all()


def test_ill_conditioned_fits_are_refused():
    cb = _bare_callback({'M2': M2})
    z = np.zeros((4, 1))
    for t in (300.0, 600.0):                                  # 2 samples for 2K + 1 = 3 unknowns
        cb.add_host_sample(t, np.zeros((4, 1, 2)), z + np.cos(M2*t))
    with pytest.raises(ValueError, match='cond'):
        cb.result()
    assert np.array_equal(cb.result(fit=False)['elev_max'], np.full(4, np.cos(M2*300.0)))
    cb = _bare_callback({'M2': M2, 'S2': S2})
    for j in range(120):                                      # 2 hours, a sample a minute: M2 and S2 need ~15 days to separate
        t = 60.0*(j + 1)
        cb.add_host_sample(t, np.zeros((4, 1, 2)), z + np.cos(M2*t) + 0.5*np.cos(S2*t))
    with pytest.raises(ValueError, match='cond') as err:
        cb.result()
    assert 'e+' in str(err.value)                             # the condition number is named
    with pytest.raises(ValueError):
        _bare_callback({'M2': M2}).result()                   # no samples at all


def _host_solver(n_steps, n_export):
    mesh = tide_mesh('triangles')
    return make_solver(mesh, Constant(0.2), dt=0.3, n_steps=n_steps, n_export=n_export)


@pytest.mark.parametrize('batch', [True, False])
def test_schedule_on_the_host_device(ref_so, monkeypatch, batch):
    """every = 3 inside the window [5 dt - , 17 dt + ]: of 20 steps the iterations 6, 9, 12, 15 are sampled.  The accumulators are,
    bit for bit, the replay of the formulas from the states of a second run without the callback; the device class has no statistics
    sets, so iterate() goes step by step without raising."""
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    dt, om = 0.3, {'M2': M2, 'S2': S2}
    s = _host_solver(20, 10)
    cb = FieldStatisticsCallback(s, harmonics=om, every=3, start_time=4.9*dt, end_time=17.1*dt, export_to_hdf5=False)
    s.add_callback(cb, eval_interval='timestep')
    if batch:
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == 20
    twin = _host_solver(20, 10)
    want = empty_accumulators((twin.mesh2d.num_cells, 3), 2)
    sampled = []
    for _ in twin.create_iterator():
        # (the generator yields before the counters move on: the state is that of iteration + 1)
        it = twin.iteration + 1
        t = it*dt
        if it % 3 == 0 and 4.9*dt <= t <= 17.1*dt:
            replay_sample(want, twin.fields.uv_2d.cell_node_values(), twin.fields.elev_2d.cell_node_values(),
                          weights_at([M2, S2], 0 + it*dt))
            sampled.append(it)
    assert sampled == [6, 9, 12, 15]
    got, n = cb.accumulators()
    assert n == cb.n_samples == 4
    assert np.array_equal(got, want)
    assert np.array_equal(s.fields.elev_2d.dat.data_ro, twin.fields.elev_2d.dat.data_ro)
    r = cb.result(fit=False)
    assert np.array_equal(r['elev_mean'], (want[3]/4).reshape(-1)) and r['uv_mean'].shape == (3*twin.mesh2d.num_cells, 2)
    f = cb.as_functions(fit=False)
    assert f['uv_mean'].function_space() is s.function_spaces.P1DGv_2d and f['elev_max'].function_space() is s.function_spaces.P1DG_2d
    assert np.array_equal(f['speed_max'].dat.data_ro, np.sqrt(want[2]).reshape(-1))


def test_export_writes_the_npz(ref_so, monkeypatch, tmp_path):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    s = _host_solver(6, 3)
    cb = FieldStatisticsCallback(s, harmonics={'M2': M2}, name='tides', outputdir=str(tmp_path))
    s.add_callback(cb, eval_interval='timestep')
    s.iterate()
    d = np.load(os.path.join(str(tmp_path), 'diagnostic_tides.npz'))
    assert int(d['n_samples']) == 6 and d['elev_max'].shape == (3*s.mesh2d.num_cells,)
    assert 'elev_amp_M2' not in d.files                       # 6 samples 0.3 s apart: no harmonic constants, the rest is written


def test_several_ranks_are_refused_at_the_first_evaluation():
    cb = _bare_callback({'M2': M2})
    cb.solver_obj.comm.size = 2
    with pytest.raises(NotImplementedError, match='several ranks'):
        cb.evaluate()


def test_abi_of_the_built_library():
    """if the library is built: the five swe2d_stats_* symbols resolve and the ABI version is still 12"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libswe2d_hip.so is not built')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('swe2d_stats_create', 'swe2d_stats_append', 'swe2d_stats_read', 'swe2d_stats_reset', 'swe2d_stats_destroy'):
        assert getattr(lib, name) is not None and name in _lib.SYMBOLS
    assert lib.swe2d_abi_version() == 12 == _lib.ABI_VERSION
