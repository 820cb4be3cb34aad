"""CPU tests of the sediment model's host side: the closures against known answers and against straight-line Python on every
branch, the Exner volume identity, the options surface and the refusals."""
import numpy as np
import pytest

from sediment_cases import D50, KS, NU, branch_state, mesh_case, ref_closures, ref_constants, threshold_margin
from thetis_amd import options as o
from thetis_amd.sediment_model import (HostSediment, SedimentModel, check_sediment_options, closures, device_parameters,
                                       sediment_constants)

RTOL = 1e-13      # numpy against libm on a handful of logarithms and powers


def _close(a, b, rtol=RTOL):
    assert abs(a - b) <= rtol*abs(b), (a, b, abs(a - b)/max(abs(b), 1e-300))


def test_known_answers():
    """the issue's values, computed from the reference's formulas in plain Python: d50 160e-6, nu 1e-6, rho_s 2650, rho0 1000,
    g 9.81, kappa 0.4, bed_reference_height 0.025, H 0.397"""
    c = sediment_constants(D50, KS, NU)
    for key, want in (('R', 1.65), ('dstar', 4.047351904034154), ('thetacr', 0.05721878308576574), ('taucr', 0.14818749318683952),
                      ('ws', 0.018098325044631047)):
        _close(c[key], want)
    out = closures(c, 0.5, 0.0, 0.397)
    for key, want in (('qfc', 0.01198957151052301), ('mu', 0.3209559246313748), ('transport_stage_param', 2.2459925660207913),
                      ('erosion_concentration', 4.2487620611242864e-04), ('rouse_number', 0.16874981421513713),
                      ('integrated_rouse', 12.122865351803975), ('erosion', 7.68954768195239e-06),
                      ('deposition', 0.21940355760924385), ('equilibrium', 3.504750682141362e-05)):
        _close(float(out[key]), want)
    out = closures(c, 0.1, 0.0, 0.397)
    assert float(out['erosion']) == 0.0
    for key, want in (('transport_stage_param', -0.8701602973591684), ('integrated_rouse', 95.28297422502729),
                      ('deposition', 1.7244622387437458)):
        _close(float(out[key]), want)


@pytest.mark.parametrize('d,branch', [(60e-6, 'dstar < 4'), (160e-6, 'dstar < 10'), (500e-6, 'dstar < 20'), (2e-3, 'dstar < 150'),
                                      (8e-3, 'else')])
def test_thetacr_and_settling_branches(d, branch):
    """thetacr in its five dstar ranges, the settling velocity in its three size ranges"""
    ref = ref_constants(d=d)
    lo, hi = {'dstar < 4': (1, 4), 'dstar < 10': (4, 10), 'dstar < 20': (10, 20), 'dstar < 150': (20, 150), 'else': (150, 1e9)}[branch]
    assert lo <= ref['dstar'] < hi
    c = sediment_constants(d, KS, NU)
    for key in ('dstar', 'thetacr', 'taucr', 'ws'):
        _close(c[key], ref[key])
    assert (d <= 1e-4, 1e-4 < d <= 1e-3, d > 1e-3).index(True) == {60e-6: 0, 160e-6: 1, 500e-6: 1, 2e-3: 2, 8e-3: 2}[d]


def test_dstar_below_one_raises():
    with pytest.raises(ValueError, match='dstar'):
        sediment_constants(10e-6, KS, NU)


@pytest.mark.parametrize('u,H,branch', [(0.5, 0.005, 'a > H'), (0.5, 3e-4, 'H <= ksp'), (0.02, 0.4, 'rouse > 3'),
                                        (None, 0.4, '|rouse| <= 1e-4'), (0.0, 0.4, 'still water'), (1.2, 0.8, 'ordinary')])
def test_closure_branches(u, H, branch):
    if u is None:       # the speed at which ustar = ws/kappa
        r = ref_closures(1.0, 0.0, H)
        u = (ref_constants()['ws']/0.4)/np.sqrt(0.5*r['qfc'])
    ref = ref_closures(0.6*u, 0.8*u, H)
    if branch == 'a > H':
        assert KS/2 > H > 3*D50
    if branch == 'H <= ksp':
        assert H <= 3*D50 and ref['mu'] == 0.0 and ref['erosion'] == 0.0
    if branch == 'rouse > 3':
        assert ref['rouse_number'] > 3
    if branch == '|rouse| <= 1e-4':
        assert abs(ref['rouse_number']) <= 1e-4
    out = closures(sediment_constants(D50, KS, NU), 0.6*u, 0.8*u, H)
    for key in ('qfc', 'mu', 'integrated_rouse', 'erosion', 'deposition', 'equilibrium', 'transport_stage_param'):
        got, want = float(out[key]), ref[key]
        assert abs(got - want) <= RTOL*abs(want), (key, got, want)


def test_branch_state_reaches_every_branch_and_sits_on_no_threshold():
    for name in ('channel', 'coast'):
        mesh = mesh_case(name)
        bath, uv, eta = branch_state(mesh, seed=1)
        H = eta + bath[mesh.cells]
        out = closures(sediment_constants(D50, KS, NU), uv[..., 0], uv[..., 1], H)
        assert (H <= 3*D50).any() and ((H > 3*D50) & (H < KS/2)).any() and (H > KS/2).any()
        assert (out['rouse_number'] > 3).any() and (np.abs(out['rouse_number']) <= 1e-4).any() and np.isinf(out['rouse_number']).any()
        assert (out['erosion'] > 0).any() and (out['erosion'] == 0).any()
        assert np.isfinite(out['erosion']).all() and np.isfinite(out['deposition']).all() and (out['deposition'] > 0).all()
        assert threshold_margin(uv[..., 0], uv[..., 1], H).min() > 1e-9
        # the vectorised closures against the straight-line ones, node by node
        for k, i in [(0, 0), (1, 2), (mesh.num_cells - 1, 1)] + [tuple(t) for t in np.argwhere(np.abs(out['rouse_number']) <= 1e-4)[:2]]:
            ref = ref_closures(uv[k, i, 0], uv[k, i, 1], H[k, i])
            for key in ('erosion', 'deposition'):
                assert abs(out[key][k, i] - ref[key]) <= RTOL*abs(ref[key])


@pytest.mark.parametrize('conservative', [False, True])
def test_exner_volume_identity(conservative):
    """one Exner update on the irregular mesh: sum_v db_v * (sum_c A_c/3) = dt*fac*sum_c A_c/3*(r_1 + r_2 + r_3), and every vertex
    against an independent scatter over the cells"""
    mesh = mesh_case('coast')
    bath, uv, eta = branch_state(mesh, seed=2, smooth=True)
    c = sediment_constants(D50, KS, NU, morfac=50.0)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c, conservative=conservative)
    E, D, eq = host.coefficients(uv, eta, bath)
    xc = mesh.vertex_xy[mesh.cells]
    S = 2.0*eq*(1.0 + 0.3*np.sin(xc[..., 0]/5e3))*(host.depth(eta, bath) if conservative else 1.0)
    dt = 0.3
    new = host.exner(E, D, S, eta, bath, dt)
    assert host.n_skipped == 0 and np.abs(new - bath).max() > 0
    r = E - (D*S/host.depth(eta, bath) if conservative else D*S)
    p = mesh.vertex_xy[mesh.cells]
    A = 0.5*np.abs((p[:, 1, 0] - p[:, 0, 0])*(p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0])*(p[:, 1, 1] - p[:, 0, 1]))
    lumped = np.zeros(len(bath))
    rhs_v = np.zeros(len(bath))
    for k in range(mesh.num_cells):                       # scatter instead of gather
        for i in range(3):
            v = mesh.cells[k, i]
            lumped[v] += A[k]/3
            rhs_v[v] += A[k]/12*(2*r[k, i] + r[k, (i + 1) % 3] + r[k, (i + 2) % 3])
    rhs = dt*c['fac']*float(np.sum(A/3*r.sum(axis=1)))
    lhs = float(np.sum((new - bath)*lumped))
    assert abs(lhs - rhs) <= 1e-12*abs(rhs), (lhs, rhs)
    want = bath + dt*c['fac']*rhs_v/lumped
    assert (np.abs(new - want) <= 1e-14*np.abs(want)).all()


def test_exner_floor_keeps_the_vertex_and_counts_it():
    mesh = mesh_case('channel')
    bath = np.full(mesh.vertex_xy.shape[0], 0.5)
    eta = np.zeros((mesh.num_cells, 3))
    eta[mesh.cells == 0] = -0.4995                      # 0.5 mm of water at vertex 0: below the 1 mm floor
    c = sediment_constants(D50, KS, NU)
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    E = np.full((mesh.num_cells, 3), 1e-5)
    new = host.exner(E, np.ones_like(E), np.zeros_like(E), eta, bath, 1.0)
    assert new[0] == bath[0] and host.n_skipped == 1 and (new[1:] > bath[1:]).all()      # erosion deepens everywhere else


def test_option_names_and_defaults():
    so = o.SedimentModelOptions()
    want = dict(solve_exner=False, solve_suspended_sediment=False, use_sediment_conservative_form=False, use_bedload=False,
                use_sediment_slide=False, horizontal_diffusivity=None, use_angle_correction=True, use_slope_mag_correction=True,
                use_secondary_current=False, average_sediment_size=None, slide_region=None, bed_reference_height=None,
                use_advective_velocity_correction=True, porosity=0.4, max_angle=32, sed_slide_length_scale=0,
                morphological_acceleration_factor=1, morphological_viscosity=None, sediment_density=2650,
                secondary_current_parameter=0.75, slope_effect_parameter=1.3, slope_effect_angle_parameter=2/3,
                check_sediment_conservation=False, check_sediment_overshoot=False, sediment_timestepper_type='CrankNicolson',
                exner_timestepper_type='CrankNicolson')
    assert set(so._all_spec()) == set(want) | {'sediment_model_class'}
    for key, v in want.items():
        got = getattr(so, key)
        assert (float(got) if isinstance(got, o.Constant) else got) == v, key
    assert so.sediment_model_class is SedimentModel
    assert list(o._SEDIMENT_STEPPERS) == ['SSPRK33', 'ForwardEuler', 'BackwardEuler', 'CrankNicolson', 'DIRK22', 'DIRK33']
    with pytest.raises(TypeError):
        so.no_such_option = 1
    m = o.ModelOptions2d()
    assert isinstance(m.sediment_model_options, o.SedimentModelOptions)
    assert m.sediment_model_options is not o.ModelOptions2d().sediment_model_options
    # set_timestepper_type sets the sediment steppers only where they are solved (options.py:1030-1035)
    m.set_timestepper_type('SSPRK33')
    assert m.sediment_model_options.sediment_timestepper_type == 'CrankNicolson'
    m.sediment_model_options.solve_suspended_sediment = True
    m.sediment_model_options.solve_exner = True
    m.set_timestepper_type('SSPRK33', use_automatic_timestep=False)
    assert m.sediment_model_options.sediment_timestepper_type == m.sediment_model_options.exner_timestepper_type == 'SSPRK33'
    assert m.sediment_model_options.sediment_timestepper_options.use_automatic_timestep is False
    assert isinstance(m.sediment_model_options.exner_timestepper_options, o.ExplicitTracerTimeStepperOptions2d)


def _options(**kw):
    m = o.ModelOptions2d()
    so = m.sediment_model_options
    so.solve_suspended_sediment = True
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    m.horizontal_viscosity = o.Constant(NU)
    so.sediment_timestepper_type = 'SSPRK33'
    so.exner_timestepper_type = 'ForwardEuler'
    for k, v in kw.items():
        setattr(so if k in so._all_spec() else m, k, v)
    return m


@pytest.mark.parametrize('kw,exc,match', [
    (dict(use_bedload=True), NotImplementedError, 'use_bedload'),
    (dict(use_sediment_slide=True), NotImplementedError, 'use_sediment_slide'),
    (dict(use_secondary_current=True), NotImplementedError, 'use_secondary_current'),
    (dict(use_advective_velocity_correction=True), NotImplementedError, 'use_advective_velocity_correction.*False'),
    (dict(solve_exner=True, use_wetting_and_drying=True), NotImplementedError, 'solve_exner.*use_wetting_and_drying'),
    (dict(use_wetting_and_drying=True), NotImplementedError, 'use_wetting_and_drying'),
    (dict(average_sediment_size=lambda x, y: 1e-4 + 0*x), NotImplementedError, 'average_sediment_size'),
    (dict(bed_reference_height=np.ones(5)), NotImplementedError, 'bed_reference_height'),
    (dict(porosity=lambda x, y: 0.4 + 0*x), NotImplementedError, 'porosity'),
    (dict(sediment_density=np.ones(5)), NotImplementedError, 'sediment_density'),
    (dict(average_sediment_size=None), ValueError, 'average_sediment_size'),
    (dict(bed_reference_height=None), ValueError, 'bed_reference_height'),
    (dict(average_sediment_size=o.Constant(10e-6)), ValueError, 'dstar'),
    (dict(horizontal_viscosity=None), ValueError, 'horizontal_viscosity'),
    (dict(horizontal_viscosity=np.ones(5)), NotImplementedError, 'horizontal_viscosity'),
    (dict(sediment_timestepper_type='CrankNicolson'), NotImplementedError, 'sediment_timestepper_type'),
    (dict(solve_exner=True, exner_timestepper_type='DIRK22'), NotImplementedError, 'exner_timestepper_type'),
])
def test_refusals_name_the_option(kw, exc, match):
    with pytest.raises(exc, match=match):
        check_sediment_options(_options(**kw))


def test_refusals_of_mesh_ranks_and_farms():
    class Quads(object):
        cells = np.zeros((4, 4), dtype=int)

    class Ranks(object):
        size = 2
    with pytest.raises(NotImplementedError, match='quadrilaterals'):
        check_sediment_options(_options(), mesh2d=Quads())
    with pytest.raises(NotImplementedError, match='ranks'):
        check_sediment_options(_options(), comm=Ranks())
    with pytest.raises(NotImplementedError, match='solve_exner.*turbine'):
        check_sediment_options(_options(solve_exner=True), tidal_farms=True)


def test_sediment_model_on_the_host():
    """SedimentModel without a device: the reference's names, terms through HostSediment, parameters of the device struct"""
    from thetis_amd.function import Function, get_functionspace
    from thetis_amd.shallowwater_eq import DepthExpression
    mesh = mesh_case('channel')
    bath, uv, eta = branch_state(mesh, seed=3, smooth=True)
    P1DG, P1DGv, P1 = (get_functionspace(mesh, 'DG', 1), get_functionspace(mesh, 'DG', 1, vector=True), get_functionspace(mesh, 'CG', 1))
    fu, fe, fb = Function(P1DGv), Function(P1DG), Function(P1)
    fu.dat.data[...] = uv.reshape(fu.dat.data.shape)
    fe.dat.data[...] = eta.reshape(fe.dat.data.shape)
    fb.dat.data[...] = bath
    opts = _options(morphological_acceleration_factor=o.Constant(10.0))
    model = SedimentModel(opts, mesh, fu, fe, DepthExpression(fb))
    model.update()
    c = sediment_constants(D50, KS, NU, morfac=10.0)
    E, D, eq = HostSediment(mesh.cells, mesh.vertex_xy, c).coefficients(uv, eta, bath)
    assert np.array_equal(model.get_erosion_term(), E) and np.array_equal(model.get_deposition_coefficient(), D)
    assert np.array_equal(model.get_equilibrium_tracer(), eq) and not model.on_device
    assert (model.dstar, model.thetacr, model.taucr, model.settling_velocity) == (c['dstar'], c['thetacr'], c['taucr'], c['ws'])
    p = model.device_parameters()
    assert p['fac'] == 10.0/(1 - 0.4) and p['a'] == KS/2 and p['ksp'] == 3*D50 and p['conservative'] == 0 and p['solve_exner'] == 0
    assert set(p) == set(device_parameters(c))


def _solver(**kw):
    from thetis_amd.function import Function, get_functionspace
    from thetis_amd.mesh import RectangleMesh
    from thetis_amd.solver2d import FlowSolver2d
    mesh = RectangleMesh(4, 3, 16.0, 1.1)
    bath = Function(get_functionspace(mesh, 'CG', 1), name='bathymetry_2d').assign(0.4)
    solver = FlowSolver2d(mesh, bath, options=None)
    solver.options.update(_options(**kw))
    solver.options.swe_timestepper_type = 'SSPRK33'
    solver.options.timestep = 0.1
    solver.options.swe_timestepper_options.use_automatic_timestep = False
    solver.options.no_exports = True
    return solver


def test_flow_solver_surface_and_refusals():
    """fields.sediment_2d, sediment_model and the sediment equation exist once the equations are built; the refusals come by name
    from there; 'equilibrium' together with 'value' raises ValueError as in the reference"""
    from thetis_amd.sediment_model import SedimentEquation2D
    solver = _solver(solve_exner=True)
    solver.create_equations()
    assert isinstance(solver.sediment_model, SedimentModel) and 'sediment_2d' in solver.fields
    assert isinstance(solver.equations.sediment, SedimentEquation2D) and 'sediment' in solver.bnd_functions
    assert solver.fields.bathymetry_2d._pull_hook is not None
    meta = solver._field_metadata()
    assert meta['sediment_2d'] == {'name': 'Sediment', 'shortname': 'Sediment', 'unit': '', 'filename': 'Sediment2d'}
    assert meta['bathymetry_2d'] == {'name': 'Bathymetry', 'shortname': 'Bathymetry', 'unit': 'm', 'filename': 'bathymetry2d'}
    with pytest.raises(NotImplementedError, match='use_bedload'):
        _solver(use_bedload=True).create_equations()
    with pytest.raises(NotImplementedError, match='CG-P1'):
        s2 = _solver(solve_exner=True)
        s2.fields.bathymetry_2d = np.full(20, 0.4)
        s2.create_fields()
        s2.create_equations()
    with pytest.raises(ValueError, match='both equilibrium and value'):
        SedimentEquation2D.check_bnd_conditions({1: {'equilibrium': None, 'value': o.Constant(1.0)}})
    SedimentEquation2D.check_bnd_conditions({1: {'equilibrium': None, 'flux': o.Constant(-0.2)}, 2: {'elev': o.Constant(0.0)}})
    with pytest.raises(NotImplementedError, match='boundary key'):
        SedimentEquation2D.check_bnd_conditions({1: {'no_such_key': 1.0}})


def test_a_run_without_sediment_options_has_no_sediment_objects():
    """no sediment field, no sediment model, no sediment equation (the step plan of such a handle is the subject of the existing
    tests/test_gpu_step_plan.py and of test_gpu_sediment.py::test_only_solve_exner_takes_the_dataflow_kernel_away)"""
    from thetis_amd.mesh import RectangleMesh
    from thetis_amd.solver2d import FlowSolver2d
    mesh = RectangleMesh(4, 3, 16.0, 1.1)
    solver = FlowSolver2d(mesh, np.full(mesh.vertex_xy.shape[0], 0.4))
    solver.options.swe_timestepper_type = 'SSPRK33'
    solver.create_equations()
    assert solver.sediment_model is None and 'sediment_2d' not in solver.fields and 'sediment' not in solver.equations
    assert not solver.options.sediment_model_options.solve_suspended_sediment
