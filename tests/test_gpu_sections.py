"""GPU tests of the section transports (csrc/swe2d_sections.hip): the device's limb sums against the numpy restatement bit for bit,
the row store, the batched time loop against the step loop, and the refusals."""
import numpy as np
import pytest

import section_cases as sc
from thetis_amd import Constant, RectangleMesh, SectionTransportCallback, _lib, sections
from thetis_amd.device import Swe2dDevice
from tide_cases import make_solver

pytestmark = pytest.mark.gpu


def _device(mesh, seed, n_tracers=2, **kw):
    uv, eta, bath, tr = sc.random_state(mesh, seed, n_tracers)
    dev = Swe2dDevice(mesh, bath, 0.05, **kw)
    dev.set_state(uv, eta)
    tids = []
    for q in tr:
        tids.append(dev.add_tracer())
        dev.tracer_set_state(tids[-1], q)
    return dev, tids, (uv, eta, bath, tr)


def _compare(dev, mesh, section_list, state, nonlinear=True, what=''):
    """eval_limbs against the host as integers; eval against the rounding of the limbs; returns the device's values"""
    uv, eta, bath, tr = state
    want, want_bad = sc.host_limbs(mesh, section_list, uv, eta, bath, tr, nonlinear)
    got, bad = dev.sections_eval_limbs()
    assert bad == want_bad == 0, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
    values, bad = dev.sections_eval()
    assert bad == 0 and np.array_equal(values, sc.values_of(want)), what
    for s, p in enumerate(section_list):
        if p is None:
            assert not got[s].any()
        else:
            assert values[s, 1] > 0.0 and np.abs(values[s, 0]) > 0.0
    return values


@pytest.fixture(scope='module')
def big(hip_lib):
    mesh = sc.big_mesh()
    section_list = sc.big_sections(mesh)
    dev, tids, state = _device(mesh, 21)
    dev.sections_set(*sc.flat(section_list), tracer_ids=tids)
    yield mesh, section_list, dev, tids, state
    dev.close()


def test_bit_for_bit_on_triangles(big):
    """40 x 30 x 2 triangles, random P1DG u, eta, two tracers, random vertex bathymetry; a diagonal of more than two workgroups, a
    one-piece section, a section through vertices and along edges, two boundary markers and an unused slot in between"""
    mesh, section_list, dev, tids, state = big
    values = _compare(dev, mesh, section_list, state, what='triangles')
    assert (np.abs(values[:4, 2:4]) > 0.0).all() and not values[:, 4:].any()
    # two appended rows equal eval; the unsummable counter is 0
    dev.sections_rows_reserve(2)
    dev.sections_rows_append()
    dev.sections_rows_append()
    rows, bad = dev.sections_rows_read()
    assert rows.shape == (2, _lib.MAX_SECTIONS, _lib.SECTION_VALUES) and not bad.any()
    assert np.array_equal(rows[0], values) and np.array_equal(rows[1], values)
    rows, bad = dev.sections_rows_read()
    assert len(rows) == 0
    with pytest.raises(_lib.Swe2dError) as err:              # the store holds two rows
        for _ in range(3):
            dev.sections_rows_append()
    assert err.value.code == _lib.ERR_INVALID_ARGUMENT
    assert len(dev.sections_rows_read()[0]) == 2


def test_bathymetry_change_is_seen(big):
    mesh, section_list, dev, tids, state = big
    uv, eta, bath, tr = state
    before, _ = dev.sections_eval()
    new = bath + np.random.default_rng(3).uniform(0.5, 2.0, bath.shape)
    dev.set_bathymetry(new)
    try:
        after = _compare(dev, mesh, section_list, (uv, eta, new, tr), what='moved bed')
        assert (after[:4, 1] > before[:4, 1]).all()
    finally:
        dev.set_bathymetry(bath)
    _compare(dev, mesh, section_list, state, what='bed restored')


def test_a_nan_is_counted_and_not_summed(big):
    mesh, section_list, dev, tids, state = big
    uv, eta, bath, tr = state
    clean, _ = dev.sections_eval()
    cell = int(section_list[1].cell[0])                       # the cell of the one-piece section ...
    others = [s for s, p in enumerate(section_list) if p is not None and cell not in set(p.cell.tolist())]
    assert 0 in others and 3 in others and 5 in others
    bad_eta = eta.copy()
    bad_eta[cell, 1] = np.nan
    dev.set_state(uv, bad_eta)
    try:
        want, want_bad = sc.host_limbs(mesh, section_list, uv, bad_eta, bath, tr)
        got, bad = dev.sections_eval_limbs()
        values, bad2 = dev.sections_eval()
    finally:
        dev.set_state(uv, eta)
    assert bad == bad2 == want_bad == 4                       # transport, area and two tracer terms of the one piece
    assert np.array_equal(got, want) and not got[1].any()     # ... is left out: its section sums nothing
    for s in others:
        assert np.array_equal(values[s], clean[s])
    _compare(dev, mesh, section_list, state, what='state restored')


@pytest.mark.parametrize('general', [False, True])
def test_boundary_sections_on_quadrilaterals(hip_lib, general):
    mesh = sc.quad_mesh(general)
    section_list = [sections.boundary_pieces(mesh, 2), None, sections.boundary_pieces(mesh, 1)]
    assert len(section_list[0]) == 33 and len(section_list[2]) == 9
    dev, tids, state = _device(mesh, 31 + general, n_tracers=1)
    try:
        dev.sections_set(*sc.flat(section_list), tracer_ids=tids)
        _compare(dev, mesh, section_list, state, what='quadrilaterals')
    finally:
        dev.close()


def test_linear_equations_take_the_bathymetry_alone(hip_lib):
    mesh = sc.big_mesh()
    section_list = sc.big_sections(mesh)[:2]
    dev, tids, state = _device(mesh, 41, n_tracers=0, use_nonlinear_equations=False)
    try:
        dev.sections_set(*sc.flat(section_list))
        _compare(dev, mesh, section_list, (state[0], state[1], state[2], []), nonlinear=False, what='linear')
    finally:
        dev.close()


def _run(monkeypatch, every, batched, flow, with_callback=True):
    """20 steps, an export every 7: (callback result, final uv, final eta, device info)"""
    monkeypatch.setenv('THETIS_AMD_FLOW', '1' if flow else '0')
    s = make_solver(RectangleMesh(12, 8, 8000.0, 4000.0), Constant(0.2), dt=0.3, n_steps=20, n_export=7, tracer=not flow)
    cb = None
    if with_callback:
        cb = SectionTransportCallback(s, {'mid': [(4100.0, -50.0), (3900.0, 4050.0)], 'open': 1},
                                      tracers=() if flow else ('tracer_2d',), every=every, append_to_log=False, export_to_hdf5=False)
        s.add_callback(cb, 'timestep')
    if batched:
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == 20
    dev = s.timestepper.device
    assert (dev.flow_supported() >= 1 and dev.get_option(_lib.OPT_FLOW) != 0) if flow else dev.get_option(_lib.OPT_FLOW) == 0
    out = (cb.result() if cb else None), s.fields.uv_2d.dat.data_ro.copy(), s.fields.elev_2d.dat.data_ro.copy()
    dev.close()                                               # (not left to the collector: the solver and its callback are a cycle)
    return out


@pytest.mark.parametrize('flow', [True, False])
@pytest.mark.parametrize('every', [1, 3])
def test_iterate_keeps_its_batches_and_the_rows_of_the_step_loop(hip_lib, monkeypatch, every, flow):
    """across two export boundaries: rows and times are bitwise those of the step loop, the final state bitwise that of a run
    without the callback - on the dataflow kernel (192 triangles, no tracer) and with SWE2D_OPT_FLOW off (a tracer along)"""
    r_b, uv_b, eta_b = _run(monkeypatch, every, True, flow)
    r_s, uv_s, eta_s = _run(monkeypatch, every, False, flow)
    _, uv_0, eta_0 = _run(monkeypatch, every, True, flow, with_callback=False)
    n = 20//every
    assert len(r_b['time']) == n and np.array_equal(r_b['time'], np.array([(every*(i + 1))*0.3 for i in range(n)]))
    for key in ('time', 'transport', 'area', 'tracer_transport', 'cumulative_volume', 'n_unsummable'):
        assert np.array_equal(r_b[key], r_s[key]), key
    assert np.isfinite(r_b['transport']).all() and (r_b['area'] > 0.0).all() and not r_b['n_unsummable'].any()
    assert r_b['tracer_transport'].shape == (n, 2, 0 if flow else 1)
    assert np.array_equal(uv_b, uv_0) and np.array_equal(eta_b, eta_0)
    assert np.array_equal(uv_s, uv_0) and np.array_equal(eta_s, eta_0)


def test_refusals(hip_lib):
    import gc
    import torch
    mesh = sc.big_mesh()
    one = sections.boundary_pieces(mesh, 1)
    dev, tids, state = _device(mesh, 51, n_tracers=1)
    n, sec, cell, w, nrm = sc.flat([one])

    def refused(code, call):
        with pytest.raises(_lib.Swe2dError) as err:
            call()
        assert err.value.code == code

    try:
        refused(_lib.ERR_INVALID_ARGUMENT, dev.sections_eval)                                      # no sections yet
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(_lib.MAX_SECTIONS + 1, sec, cell, w, nrm))
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, cell, w, nrm, tracer_ids=[0]*(_lib.MAX_SECTION_TRACERS + 1)))
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, cell, w, nrm, tracer_ids=[3]))      # no such tracer
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec + 1, cell, w, nrm))                  # slot out of range
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, np.where(np.arange(len(cell)) == 2, mesh.num_cells, cell), w, nrm))
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, np.where(np.arange(len(cell)) == 2, -1, cell), w, nrm))
        bad_w = w.copy()
        bad_w[1, 1, 2] = np.inf
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, cell, bad_w, nrm))
        bad_n = nrm.copy()
        bad_n[0, 0] = np.nan
        refused(_lib.ERR_INVALID_ARGUMENT, lambda: dev.sections_set(1, sec, cell, w, bad_n))
        dev.sections_set(n, sec, cell, w, nrm, tracer_ids=tids)
        dev.sections_rows_reserve(2)
        before = _compare(dev, mesh, [one], state, what='after the refused calls')
        # inside a stream capture: every call is refused, nothing is recorded
        s = torch.cuda.Stream()
        dev.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            buf = torch.zeros(16, device='cuda')
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            # (solvers of earlier tests are cyclic garbage that still holds device handles: a collection inside the capture would
            #  destroy them there - hipFree and a synchronisation from this thread - and invalidate the capture.  Collected now,
            #  and no collection until the capture has ended.)
            gc.collect()
            gc.disable()
            try:
                with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
                    buf.add_(1.0)                             # (the capture records something; nothing is replayed)
                    for call in (dev.sections_rows_append, dev.sections_eval, dev.sections_eval_limbs, dev.sections_rows_read,
                                 lambda: dev.sections_rows_reserve(4), dev.sections_clear,
                                 lambda: dev.sections_set(n, sec, cell, w, nrm)):
                        refused(_lib.ERR_UNSUPPORTED, call)
            finally:
                gc.enable()
            s.synchronize()
            dev.advance(1)                                    # the handle is usable
            dev.sections_rows_append()
            rows, bad = dev.sections_rows_read()
        dev.set_stream(None)
        assert len(rows) == 1 and not bad.any() and np.isfinite(rows).all() and not np.array_equal(rows[0], before)
        dev.sections_clear()
        refused(_lib.ERR_INVALID_ARGUMENT, dev.sections_rows_append)
    finally:
        dev.close()
    # a handle with wetting-drying
    dev, tids, state = _device(mesh, 52, n_tracers=0)
    try:
        dev.set_wetting_and_drying(0.5)
        dev.set_state(state[0], state[1])                     # (wetting-drying is enabled before the state is set)
        refused(_lib.ERR_UNSUPPORTED, lambda: dev.sections_set(n, sec, cell, w, nrm))
        dev.advance(1)
        assert np.isfinite(dev.get_state()[1]).all()
    finally:
        dev.close()
