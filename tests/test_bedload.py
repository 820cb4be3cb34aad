"""Bedload transport in the Exner update on the host (``-m "not gpu"``): HostSediment's nodal transport against a scalar
transcription of the reference, rest, the boundary rule on uniform flow, conservation, a migrating hump, convergence of the lumped
divergence, the open-marker rule, the option checks and the stepper's host fallback."""
import numpy as np
import pytest

from bedload_cases import (ALPHA_SECC, BETA, SURBETA2, SWITCHES, bedload_margin, bedload_state, cell_gradient, ref_bedload)
from sediment_cases import D50, KS, NU, mesh_case
from thetis_amd import options as o
from thetis_amd.function import Function, get_functionspace
from thetis_amd.mesh import RectangleMesh
from thetis_amd.sediment_model import (HostSediment, bedload_closures, bedload_constants, bedload_device_parameters,
                                       check_sediment_options, open_bedload_markers, sediment_constants)

DT = 0.05


def _constants(mag=True, ang=True, sec=True, morfac=1.0):
    return bedload_constants(sediment_constants(D50, KS, NU, morfac=morfac), BETA, SURBETA2, ALPHA_SECC, mag, ang, sec)


def _nodal_inputs(mesh, bath, uv, eta):
    hx, hy = cell_gradient(mesh, bath[mesh.cells])
    ex, ey = cell_gradient(mesh, eta)
    return uv[..., 0], uv[..., 1], eta + bath[mesh.cells], hx[:, None] + 0*eta, hy[:, None] + 0*eta, ex[:, None] + 0*eta, ey[:, None] + 0*eta


def test_state_reaches_both_sides_of_every_select():
    for name in ('channel', 'coast', 'large'):
        mesh = mesh_case(name)
        bath, uv, eta = bedload_state(mesh, seed=1)
        u, v, H, hx, hy, ex, ey = _nodal_inputs(mesh, bath, uv, eta)
        assert bedload_margin(u, v, H, hx, hy, ex, ey).min() > 1e-9
        qb = HostSediment(mesh.cells, mesh.vertex_xy, _constants()).bedload(uv, eta, bath)
        speed = np.hypot(u, v)
        moving = np.abs(qb).sum(axis=2) > 0
        assert moving.any() and (~moving & (speed > 0)).any()                 # above and below the threshold of motion
        assert (speed.max(axis=1) == 0).any()                                 # cells exactly at rest
        assert min(np.abs(g).min() for g in (hx, hy, ex, ey)) > 0                # sloping bed and surface in every cell


@pytest.mark.parametrize('mag,ang,sec', SWITCHES)
def test_nodal_transport_against_the_scalar_transcription(mag, ang, sec):
    mesh = mesh_case('channel')
    bath, uv, eta = bedload_state(mesh, seed=1)
    qb = HostSediment(mesh.cells, mesh.vertex_xy, _constants(mag, ang, sec)).bedload(uv, eta, bath)
    u, v, H, hx, hy, ex, ey = _nodal_inputs(mesh, bath, uv, eta)
    want = np.array([[ref_bedload(u[k, i], v[k, i], H[k, i], hx[k, i], hy[k, i], ex[k, i], ey[k, i], mag, ang, sec) for i in range(3)]
                     for k in range(mesh.num_cells)])
    assert np.isfinite(qb).all() and np.abs(want).max() > 0
    assert np.array_equal(qb == 0, want == 0)
    worst = np.abs(qb - want).max()/np.abs(want).max()
    print('bedload {:}: largest difference {:.3e} of max |q_b|'.format((mag, ang, sec), worst))
    assert worst <= 1e-12


@pytest.mark.parametrize('mag,ang,sec', SWITCHES)
def test_rest_gives_exact_zeros(mag, ang, sec):
    mesh = mesh_case('channel')
    bath, uv, eta = bedload_state(mesh, seed=2)
    with np.errstate(all='raise'):                  # no division, root or logarithm outside its domain on any branch
        qb = HostSediment(mesh.cells, mesh.vertex_xy, _constants(mag, ang, sec)).bedload(uv, eta, bath)
    rest = (uv == 0).all(axis=2)
    assert rest.any() and np.isfinite(qb).all() and not qb[rest].any()
    still = HostSediment(mesh.cells, mesh.vertex_xy, _constants(mag, ang, sec)).bedload(0*uv, eta, bath)
    assert not still.any() and not np.signbit(still).any()


def test_both_sides_of_the_1e_10_guards():
    """the two guards of the angle correction, which no state of bedload_state comes near, at single points: a speed whose stress
    is below 1e-10 (nothing moves: exact zeros, and the root of cparam/1e-10 is taken without complaint), and a bed slope that
    cancels the flow direction, so that the norm of the corrected direction is below 1e-10 at a MOVING node - against the scalar
    transcription, next to points on the other side of each guard"""
    import math
    from sediment_cases import G, RHO0, RHOS, ref_closures
    c = _constants(True, True, True)
    u, v, H = 0.8, 0.3, 0.4
    stress = RHO0*0.5*ref_closures(u, v, H)['qfc']*(u*u + v*v)
    tt1 = math.sqrt((RHOS - RHO0)*G*D50*SURBETA2**2/stress)
    sn = math.hypot(u, v)
    pts = [(u, v, H, -(u/sn)/tt1, -(v/sn)/tt1, 1e-3, -2e-3),                # norm ~ 1e-17 < 1e-10, moving
           (u, v, H, -0.5*(u/sn)/tt1, -(v/sn)/tt1, 1e-3, -2e-3),            # norm ~ 0.5, moving
           (1e-8, 0.0, H, 0.05, 0.02, 1e-3, -2e-3),                         # stress ~ 6e-16 < 1e-10, at rest for the threshold
           (0.2, 0.0, H, 0.05, 0.02, 1e-3, -2e-3)]                          # stress > 1e-10, below the threshold of motion
    arr = [np.array([p[j] for p in pts]) for j in range(7)]
    with np.errstate(all='raise'):
        qx, qy = bedload_closures(c, *arr)
    want = np.array([ref_bedload(*p, True, True, True) for p in pts])
    scale = np.abs(want[1]).max()
    comb = math.hypot(v/sn + tt1*pts[0][4], u/sn + tt1*pts[0][3])
    assert comb < 1e-10 < stress and RHO0*0.5*ref_closures(1e-8, 0.0, H)['qfc']*1e-16 < 1e-10
    assert scale > 0 and np.abs(want[0]).max() > 0 and not want[2:].any() and not qx[2:].any() and not qy[2:].any()
    assert np.abs(np.stack([qx, qy], axis=1) - want).max() <= 1e-12*scale


def _channel(nx=8, ny=2):
    mesh = RectangleMesh(nx, ny, 16.0, 1.1)
    n = mesh.num_cells
    bath = np.full(mesh.vertex_xy.shape[0], 0.397)
    uv = np.zeros((n, 3, 2))
    uv[..., 0] = 0.8
    return mesh, bath, uv, np.zeros((n, 3))


def test_uniform_flow_and_the_boundary_rule():
    """uniform flow along a flat channel, every correction on.  Open ends (markers 1, 2), closed walls: nothing moves.  Closed ends:
    only the end vertices change, with the sign of -q_b.n (bathymetry positive down: the closed outflow end shoals)."""
    mesh, bath, uv, eta = _channel()
    c = _constants(morfac=100.0)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    qb = host.bedload(uv, eta, bath)
    q = float(qb[0, 0, 0])
    assert q > 0 and np.ptp(qb[..., 0]) <= 1e-15*q and not qb[..., 1].any()
    dtf, h_mesh = DT*c['fac'], 1.1/2
    bound = 1e-12*dtf*q/h_mesh
    new = host.exner(None, None, None, eta, bath, DT, bedload=host.bedload_contributions(qb, mesh.cell_nbr, [1, 2]))
    assert np.abs(new - bath).max() <= bound
    closed = host.exner(None, None, None, eta, bath, DT, bedload=host.bedload_contributions(qb, mesh.cell_nbr, 0))
    x = mesh.vertex_xy[:, 0]
    inflow, outflow = x == 0.0, x == 16.0
    assert np.abs(closed - bath)[~(inflow | outflow)].max() <= bound
    assert (closed[inflow] > bath[inflow] + 1e3*bound).all() and (closed[outflow] < bath[outflow] - 1e3*bound).all()
    # an open wall lets nothing through either: q_b is parallel to it
    walls = host.exner(None, None, None, eta, bath, DT, bedload=host.bedload_contributions(qb, mesh.cell_nbr, [1, 2, 3, 4]))
    assert np.abs(walls - bath).max() <= bound


def test_closed_basin_conserves_the_bed_volume():
    mesh = mesh_case('coast')
    bath, uv, eta = bedload_state(mesh, seed=3)
    c = _constants(morfac=10.0)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    qb = host.bedload(uv, eta, bath)
    # the update from a zero bed under 10 m of water IS the bed change: no vertex is held at the floor, and no difference of two
    # beds, whose rounding (1e-16 of the bed against a change of 1e-8) would hide what is asserted
    dh = host.exner(None, None, None, np.full(eta.shape, 10.0), 0*bath, DT, bedload=host.bedload_contributions(qb, mesh.cell_nbr, 0))
    mass = np.zeros(len(bath))
    np.add.at(mass, mesh.cells.ravel(), np.repeat(host.area/3.0, 3))
    assert host.n_skipped == 0
    assert (mass*np.abs(dh)).sum() > 0 and abs((mass*dh).sum()) <= 1e-12*(mass*np.abs(dh)).sum()


def _hump_run(n_updates, dt, morfac, nx=64):
    mesh = RectangleMesh(nx, 2, 16.0, 1.1)
    x = mesh.vertex_xy[:, 0]
    bath0 = 0.4 - 0.1*np.exp(-((x - 6.0)/1.2)**2)
    c = bedload_constants(sediment_constants(D50, KS, NU, morfac=morfac), BETA, SURBETA2, ALPHA_SECC, True, True, False)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    eta = np.zeros((mesh.num_cells, 3))
    bath, first = bath0.copy(), None
    for _ in range(n_updates):
        uv = np.zeros((mesh.num_cells, 3, 2))
        uv[..., 0] = 0.26/bath[mesh.cells]                                       # u = q/H over the current bed
        qb = host.bedload(uv, eta, bath)
        bath = host.exner(None, None, None, eta, bath, dt, bedload=host.bedload_contributions(qb, mesh.cell_nbr, [1, 2]))
        first = bath.copy() if first is None else first
    return x, bath0, first, bath


def test_a_hump_migrates_downstream():
    x, bath0, first, last = _hump_run(20, 0.5, 400.0)
    up, lee = (x > 4.5) & (x < 5.7), (x > 6.3) & (x < 7.5)
    assert (first[up] > bath0[up]).all() and (first[lee] < bath0[lee]).all()    # the upstream face deepens, the lee face shoals
    centroid = lambda b: ((0.4 - b)*x).sum()/(0.4 - b).sum()
    assert np.isfinite(last).all() and centroid(last) > centroid(bath0) + 0.01
    assert (0.4 - last).max() > 0.05                                             # (it is still a hump)


def _divergence_error(nx):
    mesh = RectangleMesh(nx, nx//4, 16.0, 4.0)
    c = bedload_constants(sediment_constants(D50, KS, NU), BETA, SURBETA2, ALPHA_SECC, False, False, False)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    H0 = 0.4
    bath = np.full(mesh.vertex_xy.shape[0], H0)
    U = lambda x: 0.7 + 0.2*np.sin(2*np.pi*x/16.0)
    dU = lambda x: 0.2*(2*np.pi/16.0)*np.cos(2*np.pi*x/16.0)
    xc = mesh.vertex_xy[mesh.cells][..., 0]
    uv = np.zeros((mesh.num_cells, 3, 2))
    uv[..., 0] = U(xc)
    eta = np.zeros((mesh.num_cells, 3))
    contrib = host.bedload_contributions(host.bedload(uv, eta, bath), mesh.cell_nbr, [1, 2])
    nb, den = np.zeros(len(bath)), np.zeros(len(bath))
    np.add.at(nb, mesh.cells.ravel(), contrib.ravel())
    np.add.at(den, mesh.cells.ravel(), np.repeat(host.area/3.0, 3))
    # analytic: q = 8 (K U^2 - thetacr)^1.5 qb_scale, K from the closures at one point
    one = np.array([1.0])
    qx, _ = bedload_closures(c, one, 0*one, H0*one, 0*one, 0*one, 0*one, 0*one)
    K = ((qx[0]/(8*c['qb_scale']))**(2/3) + c['thetacr'])
    x = mesh.vertex_xy[:, 0]
    want = 12*np.sqrt(K*U(x)**2 - c['thetacr'])*c['qb_scale']*2*K*U(x)*dU(x)
    y = mesh.vertex_xy[:, 1]
    interior = (x > 0) & (x < 16.0) & (y > 0) & (y < 4.0)
    assert (K*U(x)**2 > c['thetacr']).all()
    return np.abs(nb/den - want)[interior].max(), np.abs(want).max()


def test_lumped_divergence_converges():
    e1, scale = _divergence_error(16)
    e2, _ = _divergence_error(32)
    print('lumped divergence: error {:.3e} -> {:.3e} of max {:.3e}, ratio {:.2f}'.format(e1, e2, scale, e1/e2))
    assert e1 < 0.1*scale and e1/e2 >= 3.0


class _NoFloat(object):
    pass


@pytest.mark.parametrize('bnd,want', [
    ({}, []),
    ({1: {'elev': o.Constant(0.0)}}, [1]),
    ({1: {'un': o.Constant(0.0)}}, []),
    ({1: {'un': 0}, 2: {'un': o.Constant(0.1)}}, [2]),
    ({1: {'uv': (0.0, 0.0)}, 2: {'uv': (0.5, 0.0)}}, [2]),
    ({1: {'uv': [o.Constant(0.0), o.Constant(0.0)]}}, []),
    ({1: {'elev': o.Constant(0.0), 'uv': (0.0, 0.0)}}, []),
    ({1: {'flux': o.Constant(-0.2)}, 2: {'flux': o.Constant(0.0)}}, [1]),
    ({1: {'flux': _NoFloat()}, 2: {'elev': _NoFloat(), 'un': 0.0}}, [1]),
    ({1: {}, 3: None}, [1]),
])
def test_open_marker_rule(bnd, want):
    assert sorted(open_bedload_markers(bnd)) == want
    assert sorted(open_bedload_markers(bnd, markers=[2, 3, 4])) == [m for m in want if m != 1]


def test_a_function_under_flux_counts_as_open():
    mesh = RectangleMesh(2, 2, 1.0, 1.0)
    f = Function(get_functionspace(mesh, 'DG', 1)).assign(0.0)
    assert open_bedload_markers({1: {'flux': f}, 2: {'uv': Function(get_functionspace(mesh, 'DG', 1, vector=True))}}) == [1, 2]


def _options(**kw):
    m = o.ModelOptions2d()
    so = m.sediment_model_options
    so.solve_suspended_sediment = True
    so.solve_exner = True
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    m.horizontal_viscosity = o.Constant(NU)
    so.sediment_timestepper_type = 'SSPRK33'
    so.exner_timestepper_type = 'ForwardEuler'
    for k, v in kw.items():
        setattr(so if k in so._all_spec() else m, k, v)
    return m


def test_accepted_options_give_the_bedload_constants():
    c = check_sediment_options(_options(use_bedload=True, use_secondary_current=True, slope_effect_parameter=o.Constant(1.1)))
    assert c['beta'] == 1.1 and c['surbeta2'] == 2/3 and c['alpha_secc'] == 0.75 and c['use_secondary_current']
    assert c['shields_den'] == (2650.0 - 1000.0)*9.81*D50 and c['qb_scale'] == float(np.sqrt(9.81*c['R']*D50**3))
    p = bedload_device_parameters(c)
    assert p['solve_exner'] == 1 and p['use_slope_mag_correction'] == p['use_angle_correction'] == 1 and p['fac'] == c['fac']
    assert 'beta' not in check_sediment_options(_options())


@pytest.mark.parametrize('kw,match', [
    (dict(use_bedload=True, solve_exner=False), 'use_bedload'),
    (dict(use_secondary_current=True), 'use_secondary_current'),
    (dict(use_bedload=True, use_sediment_slide=True), 'use_sediment_slide'),
    (dict(use_bedload=True, use_advective_velocity_correction=True), 'use_advective_velocity_correction'),
    (dict(use_bedload=True, use_wetting_and_drying=True), 'use_wetting_and_drying'),
    (dict(use_bedload=True, slope_effect_parameter=np.full(4, 1.3)), 'slope_effect_parameter'),
    (dict(use_bedload=True, slope_effect_angle_parameter=np.ones(4)), 'slope_effect_angle_parameter'),
    (dict(use_bedload=True, use_secondary_current=True, secondary_current_parameter=np.ones(4)), 'secondary_current_parameter'),
])
def test_refusals_name_the_option(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        check_sediment_options(_options(**kw))


def test_bedload_without_the_suspended_load_is_accepted():
    """the meander's combination; solve_exner with neither source stays refused"""
    c = check_sediment_options(_options(use_bedload=True, solve_suspended_sediment=False))
    assert c['beta'] == 1.3 and c['use_slope_mag_correction'] and c['use_angle_correction'] and not c['use_secondary_current']
    check_sediment_options(_options(use_bedload=True, solve_suspended_sediment=False, use_secondary_current=True,
                                    sediment_timestepper_type='CrankNicolson'))      # (no sediment field: its stepper is not read)
    with pytest.raises(NotImplementedError, match='solve_exner'):
        check_sediment_options(_options(solve_suspended_sediment=False))


def test_refusals_of_farms_with_bedload():
    with pytest.raises(NotImplementedError, match='solve_exner.*turbine'):
        check_sediment_options(_options(use_bedload=True), tidal_farms=True)


def test_warnings_only_without_bedload(capsys):
    from test_sediment_host import _solver
    for bedload in (False, True):
        s, uv = _solver(solve_exner=True)
        s.options.sediment_model_options.use_bedload = bedload
        s.create_equations()
        out = capsys.readouterr().out
        assert ('only applies to bedload' in out) == (not bedload)


def test_host_fallback_runs_the_bedload():
    """the stand-in device without the sediment calls, uniform flow in equilibrium along the closed 4 x 3 channel: the suspended load
    leaves the bed alone, the bedload deepens the closed inflow end and shoals the closed outflow end"""
    from test_sediment_host import DT as HDT, _solver
    s, uv = _solver(solve_exner=True, morfac=100.0)
    s.options.sediment_model_options.use_bedload = True
    s.options.simulation_end_time = 3*HDT
    s.assign_initial_conditions(uv=uv)
    model = s.sediment_model
    assert s.timestepper.tracers['sediment_2d'].host_sediment and model.use_bedload and model.open_markers() == []
    bed0 = s.fields.bathymetry_2d.dat.data_ro.copy()
    qbx, qby = model.get_bedload_term()
    assert qbx.min() > 0 and np.ptp(qbx) <= 1e-15*qbx.max() and not qby.any()
    x = s.mesh2d.vertex_xy[:, 0]
    inflow, outflow = x == 0.0, x == 16.0
    step = HDT*model.constants['fac']*float(qbx.max())/4.0                      # (q_b dt fac over the length of a cell)
    beds = [s.fields.bathymetry_2d.dat.data_ro.copy() for _ in s.create_iterator()]
    assert s.iteration == 3 and len(beds) == 3 and np.isfinite(beds[-1]).all()
    # the first update: the ends alone; afterwards the bed slopes there and the corrections answer
    assert np.abs(beds[0] - bed0)[~(inflow | outflow)].max() <= 1e-9*step
    for bed in beds:
        assert (bed[inflow] > bed0[inflow] + step).all() and (bed[outflow] < bed0[outflow] - step).all()


def test_host_fallback_without_a_sediment_field():
    """bedload only on the stand-in device: FlowSolver2d has no sediment field, the bed of the closed channel deepens at the inflow
    end and shoals at the outflow end, the first update leaves every other vertex alone; iterate() equals the generator"""
    from test_sediment_host import DT as HDT, _solver
    beds = []
    for batched in (False, True):
        s, uv = _solver(solve_exner=True, morfac=100.0)
        so = s.options.sediment_model_options
        so.solve_suspended_sediment, so.use_bedload = False, True
        s.options.simulation_end_time = 3*HDT
        s.assign_initial_conditions(uv=uv)
        model = s.sediment_model
        assert not hasattr(s.fields, 'sediment_2d') and s.timestepper.bed.host_sediment and not model.on_device
        bed0 = s.fields.bathymetry_2d.dat.data_ro.copy()
        qbx, qby = model.get_bedload_term()
        assert qbx.min() > 0 and not qby.any()
        if batched:
            s.iterate()
            beds.append(s.fields.bathymetry_2d.dat.data_ro.copy())
            continue
        steps = [s.fields.bathymetry_2d.dat.data_ro.copy() for _ in s.create_iterator()]
        x = s.mesh2d.vertex_xy[:, 0]
        inflow, outflow = x == 0.0, x == 16.0
        step = HDT*model.constants['fac']*float(qbx.max())/4.0
        assert len(steps) == 3 and np.array_equal(steps[0][~(inflow | outflow)], bed0[~(inflow | outflow)])
        for bed in steps:
            assert (bed[inflow] > bed0[inflow] + step).all() and (bed[outflow] < bed0[outflow] - step).all()
        beds.append(s.fields.bathymetry_2d.dat.data_ro.copy())
    assert np.array_equal(*beds)
