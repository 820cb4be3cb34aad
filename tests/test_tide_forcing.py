"""HarmonicTidalForcing on the host: the closed form, the nodes it writes, its validation, and - with the host stand-in device,
which has no tide table - the per-stage host evaluation that the time stepper falls back to (the stage times t + c_i dt)."""
import numpy as np
import pytest

from thetis_amd import Constant, Function, HarmonicTidalForcing, get_functionspace, solver2d
from thetis_amd import _lib
from tide_cases import CpuFacetDevice, make_forcing, make_solver, tide_mesh, tide_tables


@pytest.mark.parametrize('family', ['CG', 'DG'])
@pytest.mark.parametrize('K', [1, 3])
def test_set_tidal_field_is_the_closed_form(K, family):
    mesh = tide_mesh('triangles')
    f = make_forcing(mesh, K=K, family=family)
    fs = f.elev_field.function_space()
    om, amp, ph, mean = tide_tables(fs.node_count(), fs.node_xy(), K)
    for t in (0.0, 0.3, 44714.1, 2.6e6):
        f.set_tidal_field(t)
        want = mean.copy()
        for k in range(K):                                     # left to right, one node at a time
            want = np.array([w + a*np.cos(om[k]*t - p) for w, a, p in zip(want, amp[k], ph[k])])
        assert np.array_equal(f.elev_field.dat.data_ro, want)
    v0 = f.elev_field._host_version
    f.set_tidal_field(1.0)
    assert f.elev_field._host_version > v0                     # the time stepper uploads the field again


def test_functions_as_tables_and_scalar_mean():
    mesh = tide_mesh('quads')
    P1 = get_functionspace(mesh, 'CG', 1)
    om, amp, ph, _ = tide_tables(P1.node_count(), P1.node_xy(), 2)
    f = HarmonicTidalForcing(Function(P1), om, [Function(P1).assign(a) for a in amp], [Function(P1).assign(p) for p in ph], mean=Constant(0.25))
    g = HarmonicTidalForcing(Function(P1), om, amp, ph, mean=0.25)
    f.set_tidal_field(123.0)
    g.set_tidal_field(123.0)
    assert np.array_equal(f.elev_field.dat.data_ro, g.elev_field.dat.data_ro) and np.abs(g.elev_field.dat.data_ro).max() > 0.1


@pytest.mark.parametrize('family', ['CG', 'DG'])
def test_boundary_ids_limit_the_nodes_written(family):
    mesh = tide_mesh('triangles')
    f = make_forcing(mesh, K=3, family=family, boundary_ids=[1])
    full = make_forcing(mesh, K=3, family=family)
    f.elev_field.assign(-7.0)
    f.set_tidal_field(500.0)
    full.set_tidal_field(500.0)
    d, x = f.elev_field.dat.data_ro, f.elev_field.function_space().node_xy()[:, 0]
    on1 = np.zeros(len(d), dtype=bool)
    c, k = np.nonzero(mesh.cell_nbr == -1)
    for j in (k, (k + 1) % 3):
        on1[mesh.cells[c, j] if family == 'CG' else 3*c + j] = True
    assert on1.sum() == (5 if family == 'CG' else 8) and (x[on1] == 0.0).all()
    assert np.array_equal(d[on1], full.elev_field.dat.data_ro[on1]) and (d[~on1] == -7.0).all()


def test_validation_errors():
    mesh = tide_mesh('triangles')
    P1 = get_functionspace(mesh, 'CG', 1)
    n = P1.node_count()
    elev = Function(P1)
    K = _lib.MAX_TIDE_CONSTITUENTS + 1
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_TIDE_CONSTITUENTS'):
        HarmonicTidalForcing(elev, np.ones(K), np.ones((K, n)), np.ones((K, n)))
    with pytest.raises(ValueError):
        HarmonicTidalForcing(elev, np.ones(2), np.ones((3, n)), np.ones((2, n)))
    with pytest.raises(ValueError):
        HarmonicTidalForcing(elev, np.ones(2), np.ones((2, n)), np.ones((2, n + 1)))
    with pytest.raises(ValueError):
        HarmonicTidalForcing(elev, np.ones(2), np.ones((2, n)), np.ones((2, n)), mean=np.ones(n - 1))
    with pytest.raises(ValueError):
        HarmonicTidalForcing(elev, np.ones(1), [Function(get_functionspace(mesh, 'DG', 1))], np.ones((1, n)))
    with pytest.raises(ValueError):
        HarmonicTidalForcing(elev, np.ones(1), np.ones((1, n)), np.ones((1, n)), boundary_ids=[9])


def test_forcing_under_another_key_is_refused(ref_so, monkeypatch):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuFacetDevice, raising=False)
    mesh = tide_mesh('triangles')
    s = solver2d.FlowSolver2d(mesh, Function(get_functionspace(mesh, 'CG', 1)).assign(10.0))
    s.options.swe_timestepper_type = 'SSPRK33'
    s.options.swe_timestepper_options.use_automatic_timestep = False
    s.options.timestep = 0.3
    s.options.no_exports = True
    s.bnd_functions['shallow_water'] = {1: {'un': make_forcing(mesh, K=1, uniform=True)}}
    with pytest.raises(NotImplementedError, match="'elev'"):
        s.assign_initial_conditions()


@pytest.mark.parametrize('stepper', ['SSPRK33', 'ForwardEuler'])
def test_object_as_elev_equals_update_forcings_on_the_host_device(ref_so, monkeypatch, stepper):
    """6 steps of dt = 0.3 on the host stand-in device (no tide table: the stepper evaluates ``set_tidal_field`` itself in front of
    every stage): the object as 'elev' gives, bit for bit, the run that calls ``set_tidal_field`` from ``update_forcings`` with the
    field as 'elev' - the same numpy expression at the same stage times t_start + n*dt + c_i*dt through the same compact upload."""
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuFacetDevice, raising=False)
    mesh = tide_mesh('triangles')
    f_a = make_forcing(mesh, K=3, uniform=True)
    a = make_solver(mesh, f_a, dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    assert a.timestepper.forced_per_stage and not a.timestepper.wants_clock
    a.iterate()
    f_b = make_forcing(mesh, K=3, uniform=True)
    b = make_solver(mesh, f_b.elev_field, dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    times = []
    b.iterate(update_forcings=lambda t: (times.append(t), f_b.set_tidal_field(t)))
    assert a.iteration == b.iteration == 6 and a.simulation_time == b.simulation_time
    if stepper == 'SSPRK33':
        assert times[:6] == [0.0, 0.3, 0.15, 0.3, 0.3 + 0.3, 0.3 + 0.5*0.3] and len(times) == 18
    else:
        assert times == [k*0.3 + 0.3 for k in range(6)]
    ea, eb = a.fields.elev_2d.dat.data_ro, b.fields.elev_2d.dat.data_ro
    assert np.array_equal(ea, eb) and np.array_equal(a.fields.uv_2d.dat.data_ro, b.fields.uv_2d.dat.data_ro)
    assert np.array_equal(f_a.elev_field.dat.data_ro, f_b.elev_field.dat.data_ro)
    # ... and the tide did drive the run: the same set-up with the boundary at rest ends elsewhere
    c = make_solver(mesh, Constant(0.0), dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    c.iterate()
    assert np.abs(c.fields.elev_2d.dat.data_ro - ea).max() > 1e-6
