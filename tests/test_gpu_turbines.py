"""
Tidal turbine farms on the device: the drag term of the stage kernels against the oracle (constant thrust = a quadratic drag field)
and against tests/turbine_ref.py (table, upwind correction, support drag, several farms, wetting-drying), cells outside the farms,
the stepping paths (which decline a handle with farms), the power kernel and the batched callback.

Tolerances: TOL_RHS = 1e-12 relative L-infinity of tests/test_gpu_parity.py for a tendency; for the
difference of two tendencies the same fraction of the norm of the FULL tendency; 1e-11 after 20 steps; 1e-13 relative for the power
(a sum of positive terms added exactly, the integrand a few ulps apart).
"""
import numpy as np
import pytest

import turbine_ref as tr
from helpers import channel_case, make_oracle, make_oracle_generic, quad_case, rel_linf

pytestmark = pytest.mark.gpu

TOL_RHS = 1e-12
SPEEDS = [0.9, 1., 3., 5., 5.001]
C_T = [0.01, 0.7, 0.7, 0.1, 0.0001]


def _device(mesh, bath, dt, **kw):
    from thetis_amd.device import Swe2dDevice
    return Swe2dDevice(mesh, bath, dt, **kw)


def _case(kind, seed=0, amp_u=0.5):
    if kind == 'tri':
        mesh, bath, uv, eta = channel_case(seed=seed, amp_u=amp_u)
        orc_of = make_oracle
    else:
        mesh, bath, uv, eta = quad_case(seed=seed, amp_u=amp_u, warp=0.2 if kind == 'quad_general' else 0.0)
        orc_of = make_oracle_generic
    bath = bath + 20.0                 # deep enough for the upwind correction's radicand to stay positive (asserted in the tests)
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    inside = (xc > 30e3) & (xc < 70e3)
    assert inside.any() and not inside.all()
    return mesh, bath, uv, eta, orc_of, inside


def _density(mesh, inside, seed, scale=2e-5):
    """random P1 (continuous) density >= 0, as DG nodal values zeroed outside the farm"""
    v = scale*np.random.default_rng(100 + seed).uniform(0.2, 1.0, size=mesh.num_vertices)
    return np.where(inside[:, None], v[mesh.cells], 0.0)


def _params(farm, rho0=1000.0):
    from thetis_amd import _lib
    p = _lib.TurbineParams()
    p.support_area = farm.get('C_support', 0.0)*farm.get('A_support', 0.0)
    p.rotor_area = tr.rotor_area(farm)
    p.projected_diameter = farm.get('projected_diameter') or farm['diameter']
    p.upwind_correction = int(farm.get('upwind', False))
    p.rho0 = rho0
    if 'speeds' in farm:
        p.n_table = len(farm['speeds'])
        cp = farm.get('power_table') or [tr.default_power_coefficient(c) for c in farm['thrust_table']]
        for j in range(p.n_table):
            p.speeds[j], p.thrust[j], p.power[j] = farm['speeds'][j], farm['thrust_table'][j], cp[j]
    else:
        p.thrust_area_const = farm['thrust']*tr.rotor_area(farm)
        p.power_const = farm.get('power') or tr.default_power_coefficient(farm['thrust'])
    return p


def _set_farms(dev, farms):
    for i, f in enumerate(farms):
        dev.turbine_farm_set(i, _params(f), f['density'])


# ---- 1. identity with the oracle: a constant-thrust farm is a quadratic drag field ------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
@pytest.mark.parametrize('bottom', [None, 0.0025])
def test_constant_thrust_is_the_oracles_quadratic_drag(hip_lib, kind, bottom):
    from thetis_amd import _lib
    mesh, bath, uv, eta, orc_of, inside = _case(kind)
    eta = 0.3*eta
    farm = dict(diameter=18.0, thrust=0.8, C_support=0.7, A_support=12.0, density=_density(mesh, inside, 1))
    fric = 0.8*tr.rotor_area(farm) + 0.7*12.0
    dt = 3.0
    orc = orc_of(mesh, bath, quadratic_drag_coefficient=(bottom or 0.0) + fric/2*farm['density'], norm_smoother=0.0)
    dev = _device(mesh, bath, dt)
    if bottom is not None:
        dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, bottom)
    _set_farms(dev, [farm])
    dev.set_state(uv, eta)
    ku, ke = dev.tendency()
    ku_o, ke_o = orc.tendency(uv, eta, dt)
    print('tendency rel. Linf', kind, bottom, rel_linf(ku, ku_o), rel_linf(ke, ke_o))
    assert rel_linf(ku, ku_o) < TOL_RHS and rel_linf(ke, ke_o) < TOL_RHS
    # 20 SSPRK33 steps
    uv0, eta0 = 0.2*uv, 0.3*eta
    dev.set_state(uv0, eta0)
    dev.advance(20)
    ud, ed = dev.get_state()
    uo, eo = uv0, eta0
    for _ in range(20):
        uo, eo = orc.ssprk33_step(uo, eo, dt)
    print('20 steps rel. Linf', kind, bottom, rel_linf(ud, uo), rel_linf(ed, eo))
    assert rel_linf(ud, uo) < 1e-11 and rel_linf(ed, eo) < 1e-11
    dev.close()


# ---- 2. table, upwind correction, support drag, several farms: the farms' share of the tendency against turbine_ref ---------
def _speeds_cover_every_segment(orc, uv, inside):
    seen = []
    for phi, _, _ in orc.cell_quad:
        u_q = np.einsum('nic,i->nc', uv, phi)[inside]
        seen.append(np.hypot(u_q[:, 0], u_q[:, 1]))
    s = np.concatenate(seen)
    edges = [0.0] + SPEEDS + [np.inf]
    return all(((s >= lo) & (s < hi)).any() for lo, hi in zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
@pytest.mark.parametrize('config', ['table', 'table_upwind_support', 'two_farms', 'bottom_smoother', 'manning_wd'])
def test_farm_share_of_the_tendency(hip_lib, kind, config):
    from thetis_amd import _lib
    mesh, bath, uv, eta, orc_of, inside = _case(kind, seed=3, amp_u=1.0)
    k = mesh.cells.shape[1]
    # speeds from below cut-in to above cut-out: scale the velocity cell by cell
    scale = np.random.default_rng(5).choice([0.2, 0.95, 2.0, 4.0, 5.0005/1.4, 8.0], size=mesh.num_cells)
    uv = uv*scale[:, None, None]
    # ... and six farm cells with a uniform velocity of a chosen speed, one per segment (the last segment is 0.001 m/s wide)
    for c, sp, ang in zip(np.nonzero(inside)[0][::3], [0.5, 0.95, 2.0, 4.0, 5.0005, 7.0], [0.3, 1.1, 2.0, 2.9, 4.0, 5.5]):
        uv[c] = sp*np.array([np.cos(ang), np.sin(ang)])
    eta = 0.3*eta
    dens = _density(mesh, inside, 2)
    table = dict(diameter=18.0, speeds=SPEEDS, thrust_table=C_T, density=dens)
    kw, wd = {}, config == 'manning_wd'
    if config == 'table':
        farms = [table]
    elif config == 'table_upwind_support':
        farms = [dict(table, upwind=True, projected_diameter=20.0, C_support=0.6, A_support=10.0)]
    elif config == 'two_farms':
        farms = [dict(table, upwind=True), dict(diameter=12.0, thrust=0.6, upwind=True, density=_density(mesh, inside, 7, scale=1e-5))]
    elif config == 'bottom_smoother':
        farms = [dict(table, upwind=True)]
        kw = dict(quadratic_drag_coefficient=0.0025, norm_smoother=0.1)
    else:
        farms = [dict(table, upwind=True, C_support=0.6, A_support=10.0)]
        kw = dict(manning_drag_coefficient=0.02, use_wetting_and_drying=True, wetting_and_drying_alpha=0.5, wd_mode='nodal')
    orc = orc_of(mesh, bath, **kw)
    if wd:
        eta = orc.wd_clip_state(eta) if hasattr(orc, 'wd_clip_state') else eta
    assert _speeds_cover_every_segment(orc, uv, inside), 'the case must put lanes in every table segment'
    H = orc.nodal_depth(eta)
    for f in farms:                                               # the radicand of alpha stays positive
        if f.get('upwind'):
            worst = max(tr.thrust_area(f, s) for s in SPEEDS + [2.0])
            assert worst/((f.get('projected_diameter') or f['diameter'])*H.min()) < 1.0
    dt = 3.0
    out = []
    for with_farms in (False, True):
        dev = _device(mesh, bath, dt)
        if wd:
            dev.set_wetting_and_drying(0.5)
            dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
        if config == 'bottom_smoother':
            dev.set_scalar(_lib.SCALAR_NORM_SMOOTHER, 0.1)
            dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, 0.0025)
        if with_farms:
            _set_farms(dev, farms)
        dev.set_state(uv, eta)
        out.append(dev.tendency())
        dev.close()
    (ku0, ke0), (ku1, ke1) = out
    share = tr.drag_tendency(orc, farms, uv, eta, dt)
    err = np.abs((ku1 - ku0) - share).max()/np.abs(ku1).max()
    print('farm share', kind, config, 'error / |full tendency|', err, ' share / full', np.abs(share).max()/np.abs(ku1).max())
    assert np.abs(share).max() > 1e-6*np.abs(ku1).max()            # not vacuous
    assert err < TOL_RHS
    assert np.array_equal(ke0, ke1)
    # 3. cells outside every farm: bitwise the tendency of a handle without farms
    assert np.array_equal(ku1[~inside], ku0[~inside])


# ---- 4. paths: every stepping path declines a handle with farms and gives the bits of the stage launches ---------------------
@pytest.mark.parametrize('fused', [None, 0, 1, 2, 3])
@pytest.mark.parametrize('flow', [None, 0])
@pytest.mark.parametrize('quads', [False, True])
def test_paths_with_farms_give_the_bits_of_stage_launches(hip_lib, fused, flow, quads):
    from thetis_amd import _lib
    mesh, bath, uv, eta = quad_case(40, 16, amp_eta=0.1, amp_u=0.3) if quads else channel_case(40, 16, amp_eta=0.1, amp_u=0.3)
    bath = bath + 20.0
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    inside = (xc > 30e3) & (xc < 70e3)
    farm = dict(diameter=18.0, speeds=SPEEDS, thrust_table=C_T, upwind=True, density=_density(mesh, inside, 4))
    res = []
    for staged in (True, False):
        dev = _device(mesh, bath, 2.0)
        if fused is not None:
            dev.set_option(_lib.OPT_FUSED_STAGES, fused)
        if flow is not None:
            dev.set_option(_lib.OPT_FLOW, flow)
        dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, 0.0025)
        if not staged and not quads:
            assert dev.flow_supported() in (1, 2)                  # covered until the farm arrives
        if fused in (1, 3) and flow == 0:
            assert dev.fused_pair_info()[0]                        # the forced fused pair covers the handle until the farm arrives
        _set_farms(dev, [farm])
        assert dev.flow_supported() == 0
        assert not dev.fused_pair_info()[0] and not dev.fused_triple_info()[0] and not dev.fused_step_info()[0]
        dev.set_state(uv, eta)
        # the direct entry points of the kernels that do not carry the term refuse the handle
        for call in (lambda: dev.solve_flow([mesh.num_cells]*3), lambda: dev.solve_step_cells(mesh.num_cells)):
            with pytest.raises(_lib.Swe2dError) as err:
                call()
            assert err.value.code == _lib.ERR_UNSUPPORTED
        for _ in range(4):
            if staged:
                for i in range(3):
                    dev.solve_stage(i)
            else:
                dev.advance(1)
        res.append(dev.get_state())
        dev.turbine_farm_clear(0)
        assert quads or dev.flow_supported() in (1, 2)
        dev.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ---- 5. power ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
def test_power_against_the_reference_statement(hip_lib, kind):
    """swe2d_turbine_power against tests/turbine_ref.power at 1e-13 relative."""
    mesh, bath, uv, eta, orc_of, inside = _case(kind, seed=6, amp_u=1.0)
    scale = np.random.default_rng(8).choice([0.2, 0.95, 2.0, 4.0, 8.0], size=mesh.num_cells)
    uv = uv*scale[:, None, None]
    orc = orc_of(mesh, bath)
    farms = [dict(diameter=18.0, thrust=0.8, density=_density(mesh, inside, 1)),
             dict(diameter=18.0, speeds=SPEEDS, thrust_table=C_T, upwind=True, projected_diameter=20.0, C_support=0.6, A_support=10.0,
                  density=_density(mesh, inside, 2)),
             dict(diameter=15.0, speeds=SPEEDS, thrust_table=C_T, power_table=[0.0, 0.3, 0.45, 0.1, 0.0], density=_density(mesh, inside, 3))]
    dev = _device(mesh, bath, 3.0)
    _set_farms(dev, farms)
    dev.set_state(uv, eta)
    p = dev.turbine_power()
    limbs = dev.turbine_power_limbs()
    dev.turbine_rows_reserve(2)
    dev.turbine_rows_append()
    dev.turbine_rows_append()
    rows = dev.turbine_rows_read()
    for i, f in enumerate(farms):
        ref = tr.power(orc, f, uv)
        print('power', kind, i, p[i], ref, abs(p[i] - ref)/ref)
        assert ref > 0 and abs(p[i] - ref) <= 1e-13*ref
        assert dev.limbs_to_double(limbs[i]) == p[i]
    assert not p[len(farms):].any()
    assert rows.shape == (2, len(p)) and np.array_equal(rows[0], p) and np.array_equal(rows[1], p)
    dev.close()


def _farm_solver(tmp_path, batched, n_export=6, end_steps=18, turbines=True, dt=10.0, nx=60, ny=20):
    from thetis_amd import Constant, Function, FunctionSpace, RectangleMesh, TidalTurbineFarmOptions, solver2d, turbines as tb
    from thetis_amd.rungekutta import SSPRK33
    lx, ly = 100e3, 30e3
    mesh = RectangleMesh(nx, ny, lx, ly, cell_marker_fn=lambda x, y: np.where((x > 40e3) & (x < 60e3), 2, 0))
    calls = []
    orig = SSPRK33.advance_steps

    def counting(self, t, n, probes=None):
        calls.append(n)
        return orig(self, t, n, probes=probes)
    SSPRK33.advance_steps = counting
    try:
        P1 = FunctionSpace(mesh, 'CG', 1)
        s = solver2d.FlowSolver2d(mesh, Function(P1).assign(30.0))
        o = s.options
        o.timestep = dt
        o.simulation_export_time = n_export*dt
        o.simulation_end_time = (end_steps - 0.5)*dt
        o.no_exports = True
        o.swe_timestepper_type = 'SSPRK33'
        o.swe_timestepper_options.use_automatic_timestep = False
        o.output_directory = str(tmp_path)
        o.quadratic_drag_coefficient = Constant(0.0025)
        o.check_volume_conservation_2d = True
        s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.5)}, 2: {'elev': Constant(-0.5)}}
        if turbines:
            f = TidalTurbineFarmOptions()
            f.turbine_type = 'table'
            f.upwind_correction = True
            f.break_even_wattage = 1e3
            f.turbine_density = Function(P1).interpolate(lambda x, y: 2e-5*(1 + 0.5*np.sin(y/4e3)))
            g = TidalTurbineFarmOptions()
            g.turbine_density = Constant(1e-5)
            o.tidal_turbine_farms[2] = [f, g]
        s.create_equations()
        cb = None
        if turbines:
            cb = tb.TurbineFunctionalCallback(s, append_to_log=False, export_to_hdf5=True)
            s.add_callback(cb, 'timestep')
        s.assign_initial_conditions(elev=lambda x, y: 0.5 - x/lx, uv=Constant((1.5, 0.0)))      # above the table's cut-in speed
        if batched:
            s.iterate()
        else:
            for _ in s.create_iterator():
                pass
        return s, cb, calls
    finally:
        SSPRK33.advance_steps = orig


def test_callback_batched_equals_step_loop(hip_lib, tmp_path):
    a, cb_a, calls_a = _farm_solver(tmp_path / 'a', True)
    assert calls_a == [6]*3                                        # one advance_steps per export interval
    b, cb_b, calls_b = _farm_solver(tmp_path / 'b', False)
    assert calls_b == []
    assert len(cb_a.history) == len(cb_b.history) == 18
    assert cb_a.integrated_power == cb_b.integrated_power and cb_a.average_power == cb_b.average_power
    assert cb_a.average_profit == cb_b.average_profit and cb_a.time_period == cb_b.time_period
    assert [h[0] for h in cb_a.history] == [h[0] for h in cb_b.history]
    assert all(np.array_equal(np.array(x[1:]), np.array(y[1:])) for x, y in zip(cb_a.history, cb_b.history))
    assert min(cb_a.average_power) > 0 and cb_a.cost[1] == pytest.approx(1e-5*20e3*30e3, rel=1e-13)
    assert np.array_equal(a.fields.uv_2d.dat.data_ro, b.fields.uv_2d.dat.data_ro)
    # the history goes to diagnostic_turbine.npz at every export (in place of the HDF5 file)
    z = np.load(str(tmp_path / 'a' / 'diagnostic_turbine.npz'))
    assert z['time'].shape == (18, 1) and np.array_equal(z['time'][:, 0], [h[0] for h in cb_a.history])
    assert np.array_equal(z['average_power'], np.array([h[2] for h in cb_a.history])) and z['current_power'].shape == (18, 2)
    assert cb_a.message_str(*cb_a()).startswith('Current power, average power and profit for each farm: ')
    # a new density between two runs reaches the device
    p0 = a.tidal_farms[1].power_output()
    a.tidal_farms[1].turbine_density.assign(2e-5)
    assert a.tidal_farms[1].power_output() == pytest.approx(2*p0, rel=1e-12)


# ---- 7a. a body force cannot change the volume: closed basin with farms, the suite's 1e-12 ------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
def test_volume_is_conserved_with_farms_in_a_closed_basin(hip_lib, kind):
    from thetis_amd import _lib
    mesh, bath, uv, eta, orc_of, inside = _case(kind, seed=11, amp_u=1.5)
    farms = [dict(diameter=18.0, speeds=SPEEDS, thrust_table=C_T, upwind=True, C_support=0.6, A_support=10.0, density=_density(mesh, inside, 2)),
             dict(diameter=12.0, thrust=0.6, density=_density(mesh, inside, 7, scale=1e-5))]
    dev = _device(mesh, bath, 3.0)                                 # every boundary a closed wall
    dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, 0.0025)
    _set_farms(dev, farms)
    dev.set_state(uv, 0.3*eta)
    v0 = dev.diagnostics()[2]
    p0 = dev.turbine_power()[:2]
    dev.advance(200)
    d = dev.diagnostics()
    print('volume', kind, v0, d[2], abs(d[2] - v0)/v0, 'power before / after', p0, dev.turbine_power()[:2])
    assert np.isfinite(d).all() and p0.min() > 0
    assert abs(d[2] - v0) <= 1e-12*v0
    dev.close()


# ---- 7. physics sanity --------------------------------------------------------------------------------------------------------
def test_farm_slows_the_channel_and_power_is_below_the_kinetic_flux(hip_lib, tmp_path):
    """A channel driven by an elevation difference between its open ends, started at 1.5 m/s, with and without the farms: the flow
    inside the farm is slower with turbines; the time-averaged power is positive and below the kinetic flux 0.5 rho |u0|^3 A_T N of
    the fastest undisturbed flow (its start: the flow only decelerates; C_P / alpha^3 <= 0.72 for these turbines).  The open ends
    exchange volume: conservation to 1e-12 with farms is asserted on a closed basin, test_volume_is_conserved_with_farms_in_a_closed_basin."""
    kw = dict(n_export=150, end_steps=600, dt=8.0, nx=40, ny=8)
    with_t, cb, _ = _farm_solver(tmp_path / 'a', True, turbines=True, **kw)
    without, _, _ = _farm_solver(tmp_path / 'b', True, turbines=False, **kw)
    inside = with_t.mesh2d.cell_markers == 2

    def speeds(s):
        u = s.fields.uv_2d.dat.data_ro.reshape(-1, 3, 2)[inside]
        return np.hypot(u[..., 0], u[..., 1])
    u_t, u_0 = float(speeds(with_t).mean()), float(speeds(without).mean())
    print('mean speed in the farm with / without turbines', u_t, u_0, 'average power', cb.average_power, 'turbines', cb.cost)
    assert u_t < u_0
    a_t = np.pi*18.0**2/4
    u_max = max(1.5, float(speeds(without).max()))
    bound = 0.5*1000.0*u_max**3*a_t*sum(cb.cost)
    assert 0 < sum(cb.average_power) < bound


# ---- 8. the example ------------------------------------------------------------------------------------------------------------
def test_tidalfarm_example(hip_lib):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join('examples', 'tidalfarm.py'), '--t-end', '1200'], capture_output=True, text=True,
                       cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert any(l.startswith('Current power, average power and profit for each farm: ') for l in lines)
    last = lines[-1].split()
    assert float(last[1]) == pytest.approx(5e-5*3e3*2e3, rel=1e-12) and float(last[3]) > 0.0
