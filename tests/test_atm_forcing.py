"""Atmospheric forcing on the host: compute_wind_stress against hand-computed values, AtmosphericForcing.set_fields, the object as an
option value on the host stand-in device against the update_forcings path, and the error cases."""
import numpy as np
import pytest

from atm_cases import METHODS, atm_mesh, atm_tables, eval_times, make_atm, make_solver
from cpu_device import CpuSwe2dDevice
from thetis_amd import (AtmosphericForcing, Function, compute_wind_stress, get_functionspace, physical_constants, solver2d)


def test_rho_air_is_the_references():
    assert float(physical_constants['rho_air']) == 1.22


def test_compute_wind_stress_hand_values():
    """both branches of each formulation, worked by hand in the documented order (m = sqrt(u*u + v*v); m6 = (m*m)*(m*m)*(m*m);
    tau = C_D*rho_air*m; tau_x = tau*u)"""
    rho = 1.22
    # (3, 4): m = 5 exactly; (21, 28): m = 35 exactly
    u, v = np.array([3.0, 21.0, 0.0]), np.array([4.0, 28.0, 0.0])
    m6 = (5.0*5.0)*(5.0*5.0)*(5.0*5.0)
    cd5 = 1.e-3*(2.7/(5.0 + 1e-3) + 0.142 + 5.0/13.09 - 3.14807e-10*m6)
    tx, ty = compute_wind_stress(u, v)                                     # LargeYeager2009 is the default
    assert tx[0] == cd5*rho*5.0*3.0 and ty[0] == cd5*rho*5.0*4.0
    assert tx[1] == 2.34e-3*rho*35.0*21.0 and ty[1] == 2.34e-3*rho*35.0*28.0      # capped above 33 m/s
    assert abs(cd5 - 1.063858e-3) < 1e-9                                   # 0.539892 + 0.142 + 0.381971 - 0.000005, by hand
    # independent literals, worked on paper: 2.34e-3 * 1.22 * 35 * 21 = 2.098278; 1.0638581e-3 * 1.22 * 5 * 3 = 0.01946860
    assert abs(tx[1] - 2.098278) < 1e-12 and abs(ty[1] - 2.797704) < 1e-12
    assert abs(tx[0] - 0.01946860) < 1e-8
    assert tx[2] == 0.0 and ty[2] == 0.0
    tx, ty = compute_wind_stress(u, v, method='LargePond1981')
    assert tx[0] == 1.2e-3*rho*5.0*3.0 and ty[0] == 1.2e-3*rho*5.0*4.0            # below 11 m/s
    cd35 = 1.0e-3*(0.49 + 0.065*35.0)
    assert tx[1] == cd35*rho*35.0*21.0 and ty[1] == cd35*rho*35.0*28.0 and abs(cd35 - 2.765e-3) < 1e-15
    assert tx[2] == 0.0 and ty[2] == 0.0
    tx, ty = compute_wind_stress(u, v, method='SmithBanke1975')
    assert tx[0] == (0.63 + 0.066*5.0)/1000.*rho*5.0*3.0 and abs(tx[0] - 0.96e-3*rho*15.0) < 1e-15
    assert ty[1] == (0.63 + 0.066*35.0)/1000.*rho*35.0*28.0
    assert tx[2] == 0.0 and ty[2] == 0.0
    # the reference's own expression (numpy.hypot, **6) agrees to round-off
    m = np.hypot(u, v)
    ref = 1.e-3*(2.7/(m + 1e-3) + 0.142 + m/13.09 - 3.14807e-10*m**6)
    ref[m > 33.0] = 2.34e-3
    assert np.allclose(compute_wind_stress(u, v)[0], ref*rho*m*u, rtol=1e-14, atol=0.0)
    with pytest.raises(ValueError):
        compute_wind_stress(u, v, method='Charnock')


@pytest.mark.parametrize('n_t', [2, 5])
@pytest.mark.parametrize('method', METHODS)
def test_set_fields(n_t, method):
    mesh = atm_mesh('tri280')
    f = make_atm(mesh, n_t=n_t, method=method)
    times, u, v, p = atm_tables(mesh, n_t)
    # at the snapshot times the snapshots themselves
    for k in sorted({0, n_t//2, n_t - 1}):
        f.set_fields(times[k])
        tx, ty = compute_wind_stress(u[k], v[k], method=method)
        assert np.array_equal(f.wind_stress_field.dat.data_ro, np.stack([tx, ty], axis=1))
        assert np.array_equal(f.atm_pressure_field.dat.data_ro, p[k])
    # midpoints: the weighted mean of the two snapshots, the weight about one half
    for j in range(n_t - 1):
        t = 0.5*(times[j] + times[j + 1])
        al = (t - times[j])/(times[j + 1] - times[j])
        assert abs(al - 0.5) < 1e-15
        f.set_fields(t)
        assert np.array_equal(f.atm_pressure_field.dat.data_ro, (1.0 - al)*p[j] + al*p[j + 1])
        tx, ty = compute_wind_stress((1.0 - al)*u[j] + al*u[j + 1], (1.0 - al)*v[j] + al*v[j + 1], method=method)
        assert np.array_equal(f.wind_stress_field.dat.data_ro, np.stack([tx, ty], axis=1))
        assert np.abs(f.atm_pressure_field.dat.data_ro - 0.5*(p[j] + p[j + 1])).max() < 1e-9
    # off the grid: the weights of the bracket
    t = eval_times(times)[3]
    j, alpha = f.bracket(t)
    assert times[j] <= t < times[j + 1] and alpha == (t - times[j])/(times[j + 1] - times[j])
    f.set_fields(t)
    assert np.array_equal(f.atm_pressure_field.dat.data_ro, (1.0 - alpha)*p[j] + alpha*p[j + 1])
    assert np.abs(f.wind_stress_field.dat.data_ro).max() > 1.0 and (f.wind_stress_field.dat.data_ro[mesh.vertex_xy[:, 0] == 0.0] == 0.0).all()


def test_hpa_and_single_quantities():
    mesh = atm_mesh('triangles')
    pa, hpa = make_atm(mesh, wind=False), make_atm(mesh, wind=False, units='hpa')
    assert hpa.wind_stress_field is None and hpa.which == 2
    for t in eval_times(pa.times):
        pa.set_fields(t)
        hpa.set_fields(t)
        a, b = pa.atm_pressure_field.dat.data_ro, hpa.atm_pressure_field.dat.data_ro
        assert np.abs(a).min() > 9e4 and np.abs(a - b).max() <= 1e-10*np.abs(a).max()
    hpa.set_fields(0.0)
    assert np.array_equal(hpa.atm_pressure_field.dat.data_ro, (atm_tables(mesh)[3][0]/100.0)*100)
    w = make_atm(mesh, pressure=False)
    assert w.atm_pressure_field is None and w.which == 1
    w.set_fields(1.0)
    assert np.abs(w.wind_stress_field.dat.data_ro).max() > 1.0


def test_times_outside_the_record():
    mesh = atm_mesh('triangles')
    f = make_atm(mesh, n_t=5)
    t0, t1 = float(f.times[0]), float(f.times[-1])
    for t in (t0 - 0.1, t1 + 0.1, -1e30, np.nan):
        with pytest.raises(ValueError) as err:
            f.set_fields(t)
        assert repr(float(t)) in str(err.value) and repr(t0) in str(err.value) and repr(t1) in str(err.value)
    # the reference's RELTOL = 1e-6 of slack on alpha, clamped: the end snapshots themselves
    f.set_fields(t1 + 1e-7*(t1 - f.times[-2]))
    assert np.array_equal(f.atm_pressure_field.dat.data_ro, f.pressure[-1])
    f.set_fields(t0 - 1e-7*(f.times[1] - t0))
    assert np.array_equal(f.atm_pressure_field.dat.data_ro, f.pressure[0])


def test_validation_errors():
    mesh = atm_mesh('triangles')
    times, u, v, p = atm_tables(mesh, 5)
    ws = Function(get_functionspace(mesh, 'CG', 1, vector=True))
    pa = Function(get_functionspace(mesh, 'CG', 1))
    AtmosphericForcing(ws, pa, times, u, v, p)
    for args, kw in (((None, None, times, u, v, p), {}),
                     ((pa, pa, times, u, v, p), {}),                               # a scalar field for the stress
                     ((ws, ws, times, u, v, p), {}),
                     ((ws, Function(get_functionspace(mesh, 'DG', 1)), times, u, v, p), {}),
                     ((ws, pa, times[:1], u[:1], v[:1], p[:1]), {}),               # one snapshot
                     ((ws, pa, times[::-1], u, v, p), {}),                         # not increasing
                     ((ws, pa, np.array([0.0, 1.0, 1.0, 2.0, 3.0]), u, v, p), {}),
                     ((ws, pa, times, u[:, :-1], v, p), {}),                       # not one value per vertex
                     ((ws, pa, times, u, v, p[:-1]), {}),
                     ((ws, pa, times, u, None, p), {}),
                     ((ws, pa, times, u, v, np.where(p > 0, np.nan, p)), {}),
                     ((ws, pa, times, u, v, p), {'method': 'Charnock'}),
                     ((ws, pa, times, u, v, p), {'pressure_units': 'bar'}),
                     ((ws, Function(get_functionspace(atm_mesh('quads'), 'CG', 1)), times, u, v, p), {})):
        with pytest.raises(ValueError):
            AtmosphericForcing(*args, **kw)


def test_option_value_rules(ref_so, monkeypatch):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    mesh = atm_mesh('triangles')
    both, wind_only, pressure_only = make_atm(mesh), make_atm(mesh, pressure=False), make_atm(mesh, wind=False)
    with pytest.raises(ValueError):                                                # no wind_stress_field under options.wind_stress
        make_solver(mesh, pressure_only, None).create_timestepper()
    with pytest.raises(ValueError):
        make_solver(mesh, None, wind_only).create_timestepper()
    with pytest.raises(NotImplementedError):                                       # two different objects
        make_solver(mesh, both, make_atm(mesh)).create_timestepper()
    with pytest.raises(ValueError):                                                # tables of another mesh's vertex count
        make_solver(mesh, make_atm(atm_mesh('tri280')), None).create_timestepper()


@pytest.mark.parametrize('which', ['wind', 'pressure', 'both'])
@pytest.mark.parametrize('stepper', ['SSPRK33', 'ForwardEuler'])
def test_object_as_option_equals_update_forcings_on_the_host_device(ref_so, monkeypatch, stepper, which):
    """6 steps of dt = 0.3 on the host stand-in device (no ``atm_set``: the stepper calls ``set_fields`` itself in front of every
    stage): the object as option value gives, bit for bit, the run that calls ``set_fields`` from ``update_forcings`` with the two
    fields as option values - the same numpy expressions at the same stage times through the same per-vertex upload."""
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    mesh = atm_mesh('triangles')
    kw = dict(wind=which != 'pressure', pressure=which != 'wind')
    f_a = make_atm(mesh, **kw)
    a = make_solver(mesh, f_a if kw['wind'] else None, f_a if kw['pressure'] else None, dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    a.create_timestepper()
    assert a.timestepper.forced_per_stage and not a.timestepper.wants_clock
    a.iterate()
    f_b = make_atm(mesh, **kw)
    b = make_solver(mesh, f_b.wind_stress_field, f_b.atm_pressure_field, dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    times = []
    b.iterate(update_forcings=lambda t: (times.append(t), f_b.set_fields(t)))
    assert a.iteration == b.iteration == 6 and a.simulation_time == b.simulation_time
    if stepper == 'SSPRK33':
        assert times[:6] == [0.0, 0.3, 0.15, 0.3, 0.3 + 0.3, 0.3 + 0.5*0.3] and len(times) == 18
    else:
        assert times == [k*0.3 + 0.3 for k in range(6)]
    ea, eb = a.fields.elev_2d.dat.data_ro, b.fields.elev_2d.dat.data_ro
    assert np.isfinite(ea).all() and np.array_equal(ea, eb) and np.array_equal(a.fields.uv_2d.dat.data_ro, b.fields.uv_2d.dat.data_ro)
    # ... and the forcing did drive the run: the same set-up without it ends elsewhere
    c = make_solver(mesh, None, None, dt=0.3, n_steps=6, n_export=3, stepper=stepper)
    c.iterate()
    assert np.abs(c.fields.elev_2d.dat.data_ro - ea).max() > 1e-7
