"""The sediment slide on the host (``-m "not gpu"``): ``HostSediment.slide`` against a scalar transcription of the reference's
``get_sediment_slide_term`` and the volume integral of ``ExnerSedimentSlideTerm`` (tests/slide_cases.py), conservation, the ramp of
the reference's ``test/sediment/test_sed_slide.py`` at rest, the flags, the option checks and the host fallback of the steppers."""
import numpy as np
import pytest

from sediment_cases import D50, KS, NU, mesh_case
from slide_cases import (DT, LENGTH, MAX_ANGLE, MORFAC, POROSITY, RAMP_ANGLE, TANPHI, ramp_bed, ramp_mesh, ref_slide, slide_c,
                         steep_bed)
from thetis_amd import options as o
from thetis_amd.function import Function, get_functionspace
from thetis_amd.sediment_model import HostSediment, check_sediment_options, slide_constants, slide_device_parameters

EPS = np.finfo(np.float64).eps

# Largest difference of alpha between HostSediment.slide and the scalar transcription, relative to max |alpha|, over the cases of
# test_slide_against_the_transcription: channel 2.8e-15 (seed 2), 2.9e-15 (seed 4); coast 1.8e-14 (seed 5), 1.4e-14 (seed 7); the
# contributions 2.7e-15 / 2.6e-15 / 1.5e-14 / 1.3e-14 of max |c|; beta to 9.8e-15 rad.  The two sides form the gradient of the bed
# differently (hat-gradient table against Cramer's rule on differences), and 1/cos(beta*dt*morfac) = 1/cos(2 beta) amplifies that
# rounding by 2 tan(2 beta) <= 14 below the 41 degrees the cases keep to.
# Asserted: ten times the largest, capped at the 1e-12 that tells a wrong formula from rounding.
MEASURED_ALPHA = 1.9e-14
ALPHA_BOUND = min(10*MEASURED_ALPHA, 1e-12)


def _volume(host, bath):
    """the lumped bed volume sum_v den_v b_v, den_v the lumped mass of the vertex (a third of the area of its cells)"""
    den = np.zeros(host.n_vertices)
    np.add.at(den, host.cells.ravel(), np.repeat(host.area/3.0, 3))
    return float((den*bath).sum()), float((den*np.abs(bath)).sum())


@pytest.mark.parametrize('name,seed', [('channel', 2), ('channel', 4), ('coast', 5), ('coast', 7)])
def test_slide_against_the_transcription(name, seed):
    mesh = mesh_case(name)
    bath = steep_bed(mesh, seed)
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c())
    alpha, beta, contrib, flagged = host.slide(bath, DT)
    ra, rb, rc = ref_slide(mesh, bath, DT)
    active = alpha != 0
    assert 0.35 < active.mean() < 0.65 and np.array_equal(active, ra != 0)       # roughly half the cells slide, the same ones
    assert np.degrees(rb.max()) < 41.0 and flagged == 0                          # (away from the zero of the reference's cosine)
    assert (alpha <= 0).all() and np.isfinite(alpha).all()
    ea = np.abs(alpha - ra).max()/np.abs(ra).max()
    ec = np.abs(contrib - rc).max()/np.abs(rc).max()
    eb = np.abs(beta - rb).max()
    print('slide {:} seed {:}: alpha {:.3e} of max |alpha|, contributions {:.3e} of max |c|, beta {:.3e} rad'.format(name, seed, ea, ec, eb))
    assert ea <= ALPHA_BOUND and ec <= ALPHA_BOUND and eb <= ALPHA_BOUND


@pytest.mark.parametrize('name', ['channel', 'coast'])
def test_region_scales_the_slope_test_only(name):
    """a per-cell region: the transcription agrees, cells with region 0 do not slide, and the contributions keep the unscaled gradient"""
    mesh = mesh_case(name)
    bath = steep_bed(mesh, 2)
    region = np.where(np.arange(mesh.num_cells) % 2 == 0, 0.0, 1.0)
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c())
    alpha, beta, contrib, _ = host.slide(bath, DT, region)
    ra, rb, rc = ref_slide(mesh, bath, DT, region)
    assert not alpha[::2].any() and not beta[::2].any() and alpha[1::2].any()
    assert np.abs(alpha - ra).max() <= ALPHA_BOUND*np.abs(ra).max() and np.abs(contrib - rc).max() <= ALPHA_BOUND*np.abs(rc).max()
    full = host.slide(bath, DT)
    assert np.array_equal(alpha[1::2], full[0][1::2]) and np.array_equal(contrib[1::2], full[2][1::2])
    half = host.slide(bath, DT, np.full(mesh.num_cells, 0.5))
    assert np.array_equal(half[2], host.slide_contributions(half[0], bath)) and (half[0] != full[0]).any()


@pytest.mark.parametrize('name', ['channel', 'coast'])
def test_contributions_sum_to_zero_and_the_volume_is_conserved(name):
    """Per cell c_0 + c_1 + c_2 = 0 up to rounding.  c_i = fl(fl(A alpha) fl(fl(gx_i bx) + fl(gy_i by))) carries at most 4 eps of
    |A alpha| (|gx_i bx| + |gy_i by|), the two additions 2 eps of the partial sums, and the rounded table entries add up to zero to
    1.5 eps of the largest: 8 eps of  A |alpha| sum_i (|gx_i bx| + |gy_i by|)  bounds the sum.  On these two meshes that is within
    8 ulp of A |alpha| |grad b|^2 as well (measured: 4.0 on the channel, 0.01 on the coast).
    The lumped volume over 50 updates: every update rounds b_v once and the gather of den_v and of the contributions a few times; 4 eps
    of sum_v den_v |b_v| per step bounds the drift (measured: 0 on both meshes)."""
    mesh = mesh_case(name)
    bath = steep_bed(mesh, 2)
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c())
    alpha, beta, contrib, _ = host.slide(bath, DT)
    bx, by = host.gradient(bath[mesh.cells])
    scale = host.area*np.abs(alpha)*sum(np.abs(host.grad_x[:, i]*bx) + np.abs(host.grad_y[:, i]*by) for i in range(3))
    total = np.abs((contrib[:, 0] + contrib[:, 1]) + contrib[:, 2])
    assert alpha.any() and (total <= 8*EPS*scale).all()
    ulp = total[alpha != 0]/(EPS*(host.area*np.abs(alpha)*(bx*bx + by*by))[alpha != 0])
    print('slide {:}: contributions sum to {:.2f} ulp of A |alpha| |grad b|^2 at most'.format(name, ulp.max()))
    assert ulp.max() <= 8.0
    eta = np.full((mesh.num_cells, 3), 0.5)
    v0, scale_v = _volume(host, bath)
    b, steps = bath, 50
    for _ in range(steps):
        b = host.exner(None, None, None, eta, b, DT, slide=host.slide(b, DT)[2])
    drift = abs(_volume(host, b)[0] - v0)/scale_v
    print('slide {:}: volume drift {:.3e} over {:d} steps'.format(name, drift, steps))
    assert host.n_skipped == 0 and np.abs(b - bath).max() > 0 and drift <= 4*EPS*steps


def ramp_run(n_steps, dt=DT, morfac=MORFAC):
    """the ramp at rest, slide only: (angles in degrees before every step and after the last, flagged passes, relative volume drift)"""
    mesh = ramp_mesh()
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c(morfac=morfac))
    eta = np.full((mesh.num_cells, 3), 4.0)
    b = ramp_bed(mesh)
    v0, scale = _volume(host, b)
    angles, flagged = [], 0
    for _ in range(n_steps):
        alpha, beta, contrib, fl = host.slide(b, dt)
        angles.append(float(np.degrees(beta.max())))
        flagged += fl
        b = host.exner(None, None, None, eta, b, dt, slide=contrib)
    angles.append(float(np.degrees(host.slide(b, dt)[1].max())))
    assert host.n_skipped == 0
    return np.array(angles), flagged, abs(_volume(host, b)[0] - v0)/scale


def test_the_ramp_of_the_reference_test_relaxes_to_the_angle_of_repose():
    """dt = 0.1, morfac = 20, porosity = 0.4, L = 0.2, 22 degrees: 26.565 degrees at the start, 24.72 after 200 steps, 22.013 after
    2000 and never below 22; the maximum angle never increases; no cell flagged; volume drift 2.2e-16"""
    angles, flagged, drift = ramp_run(2000)
    print('ramp: {:.4f} -> {:.4f} (200) -> {:.4f} (2000), flagged {:d}, drift {:.3e}'.format(angles[0], angles[200], angles[2000], flagged, drift))
    assert abs(angles[0] - RAMP_ANGLE) < 1e-9 and abs(angles[0] - 26.565) < 1e-3
    assert (np.diff(angles) <= 0).all()
    assert 24.5 < angles[200] < 25.0
    assert 22.0 <= angles[2000] < 22.1 and angles.min() >= 22.0
    assert flagged == 0 and drift < 1e-15


def test_a_negative_cosine_and_a_step_above_the_bound_are_flagged_not_refused():
    mesh = ramp_mesh()
    bath = ramp_bed(mesh)
    steep = int((np.abs(HostSediment(mesh.cells, mesh.vertex_xy, slide_c()).gradient(bath[mesh.cells])[0]) > 0.4).sum())
    # beta dt morfac = 0.4636*0.1*200 = 9.27, cos < 0: alpha > 0 in every cell of the ramp
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c(morfac=200.0))
    alpha, _, contrib, flagged = host.slide(bath, DT)
    assert steep == 200 and flagged == steep and (alpha[alpha != 0] > 0).all() and np.isfinite(contrib).all()
    # morfac = 0.01, dt = 10: the cosine is 1 to 1e-3, alpha = -2.1e-3 < 0, and dt |alpha| 3 max |grad psi|^2 = 10*2.1e-3*3*50 = 3.1 > 1
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c(morfac=0.01))
    alpha, _, _, flagged = host.slide(bath, 10.0)
    assert flagged == steep and (alpha <= 0).all() and alpha.min() < -1e-3
    assert host.slide(bath, 1.0)[3] == 0                                         # (the same slide at a step below the bound)


def _options(**kw):
    m = o.ModelOptions2d()
    so = m.sediment_model_options
    so.solve_suspended_sediment = True
    so.solve_exner = True
    so.use_sediment_slide = True
    so.sed_slide_length_scale = o.Constant(LENGTH)
    so.max_angle = o.Constant(MAX_ANGLE)
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    m.horizontal_viscosity = o.Constant(NU)
    so.sediment_timestepper_type = 'SSPRK33'
    so.exner_timestepper_type = 'ForwardEuler'
    for k, v in kw.items():
        setattr(so if k in so._all_spec() else m, k, v)
    return m


def test_accepted_options_give_the_slide_constants():
    c = check_sediment_options(_options(morphological_acceleration_factor=o.Constant(MORFAC)))
    assert c['tanphi'] == TANPHI and c['slide_length_scale'] == LENGTH and c['porosity'] == POROSITY and c['morfac'] == MORFAC
    assert c == slide_c()
    p = slide_device_parameters(c)
    assert p == dict(tanphi=TANPHI, length_scale=LENGTH, porosity=POROSITY, morfac=MORFAC, fac=MORFAC/(1 - POROSITY), min_depth=1e-3,
                     solve_exner=1)
    for kw in (dict(use_bedload=True), dict(solve_suspended_sediment=False), dict(solve_suspended_sediment=False, use_bedload=True),
               dict(exner_timestepper_type='SSPRK33'), dict(slide_region=o.Constant(1.0))):
        assert 'tanphi' in check_sediment_options(_options(**kw))
    assert 'tanphi' not in check_sediment_options(_options(use_sediment_slide=False))
    assert slide_constants({}, 45.0, 1.0)['tanphi'] == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize('kw,match', [
    (dict(solve_exner=False), 'use_sediment_slide without solve_exner'),
    (dict(max_angle=np.full(4, 22.0)), 'max_angle'),
    (dict(sed_slide_length_scale=np.full(4, 0.2)), 'sed_slide_length_scale'),
    (dict(sed_slide_length_scale=o.Constant(0.0)), 'use_sediment_slide.*sed_slide_length_scale'),
    (dict(porosity=lambda x, y: 0.4 + 0*x), 'porosity'),
    (dict(slide_region=lambda x, y: 1.0 + 0*x), 'slide_region'),
    (dict(slide_region=np.ones(7)), 'slide_region'),
    (dict(use_wetting_and_drying=True), 'use_wetting_and_drying'),
    (dict(exner_timestepper_type='CrankNicolson'), 'exner_timestepper_type'),
])
def test_refusals_name_the_option(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        check_sediment_options(_options(**kw))


def test_refusals_of_mesh_ranks_farms_and_regions():
    class Quads(object):
        cells = np.zeros((4, 4), dtype=int)

    class Ranks(object):
        size = 2
    with pytest.raises(NotImplementedError, match='quadrilaterals'):
        check_sediment_options(_options(), mesh2d=Quads())
    with pytest.raises(NotImplementedError, match='ranks'):
        check_sediment_options(_options(), comm=Ranks())
    with pytest.raises(NotImplementedError, match='solve_exner.*turbine'):
        check_sediment_options(_options(solve_suspended_sediment=False), tidal_farms=True)
    mesh = ramp_mesh()
    for space in (get_functionspace(mesh, 'DG', 1), get_functionspace(mesh, 'CG', 1, vector=True)):
        with pytest.raises(NotImplementedError, match='slide_region'):
            check_sediment_options(_options(slide_region=Function(space)), mesh2d=mesh)


def test_slide_region_is_one_number_per_cell():
    from thetis_amd.sediment_model import _slide_region
    mesh = ramp_mesh()
    assert _slide_region(None, mesh) is None
    assert np.array_equal(_slide_region(o.Constant(0.5), mesh), np.full(mesh.num_cells, 0.5))
    dg0 = Function(get_functionspace(mesh, 'DG', 0))
    dg0.dat.data[...] = np.arange(mesh.num_cells)
    assert np.array_equal(_slide_region(dg0, mesh), np.arange(mesh.num_cells, dtype=float))
    cg = Function(get_functionspace(mesh, 'CG', 1))
    cg.dat.data[...] = mesh.vertex_xy[:, 0]
    v = mesh.vertex_xy[mesh.cells][..., 0]
    assert np.array_equal(_slide_region(cg, mesh), ((v[:, 0] + v[:, 1]) + v[:, 2])/3.0)


def _fallback_solver(with_sediment, slide=True, n_steps=5):
    from test_sediment_host import HostSedimentDevice
    from thetis_amd.mesh import RectangleMesh
    from thetis_amd.solver2d import FlowSolver2d
    mesh = RectangleMesh(8, 2, 4.0, 1.0)
    x = mesh.vertex_xy[:, 0]
    bath = Function(get_functionspace(mesh, 'CG', 1), name='bathymetry_2d').assign(1.0 + np.where(x < 2.0, 0.0, 0.5*x - 1.0))
    s = FlowSolver2d(mesh, bath)
    s._device_cls = HostSedimentDevice
    m, so = s.options, s.options.sediment_model_options
    so.solve_suspended_sediment = with_sediment
    so.solve_exner = True
    so.use_sediment_slide = slide
    so.use_bedload = not slide and not with_sediment
    so.sed_slide_length_scale = o.Constant(LENGTH)
    so.max_angle = o.Constant(MAX_ANGLE)
    so.morphological_acceleration_factor = o.Constant(MORFAC)
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    so.morphological_viscosity = o.Constant(NU)
    m.horizontal_viscosity = None
    m.no_exports = True
    m.set_timestepper_type('SSPRK33')
    so.exner_timestepper_type = 'ForwardEuler'
    for t in (m.swe_timestepper_options, m.tracer_timestepper_options, so.sediment_timestepper_options):
        if hasattr(t, 'use_automatic_timestep'):
            t.use_automatic_timestep = False
    m.timestep = DT
    m.simulation_export_time = 100*DT
    m.simulation_end_time = n_steps*DT
    return s, mesh


def test_host_fallback_moves_the_bed_as_host_sediment_does():
    """slide alone on the stand-in device at rest: the beds of the generator are those of the HostSediment loop, bit for bit;
    iterate() equals the generator; the model's surface reads the host pass"""
    s, mesh = _fallback_solver(False)
    s.assign_initial_conditions()
    model = s.sediment_model
    assert s.timestepper.bed.host_sediment and not model.on_device and not hasattr(s.fields, 'sediment_2d')
    assert model.max_slope_angle() == pytest.approx(RAMP_ANGLE, abs=1e-9) and model.slide_flagged() == 0
    host = HostSediment(mesh.cells, mesh.vertex_xy, slide_c())
    b = s.fields.bathymetry_2d.dat.data_ro.copy()
    a0 = host.slide(b, DT)
    assert np.array_equal(model.get_sediment_slide_term().dat.data_ro, a0[0]) and np.array_equal(model.betaangle.dat.data_ro, a0[1])
    assert model.betaangle.function_space().family == 'DG' and model.betaangle.function_space().degree == 0
    want = []
    for _ in range(5):
        b = host.exner(None, None, None, np.zeros((mesh.num_cells, 3)), b, DT, slide=host.slide(b, DT)[2])
        want.append(b)
    got = [s.fields.bathymetry_2d.dat.data_ro.copy() for _ in s.create_iterator()]
    assert len(got) == 5 and all(np.array_equal(p, q) for p, q in zip(got, want)) and np.abs(got[-1] - got[0]).max() > 0
    assert model.max_slope_angle() == np.degrees(host.slide(want[-2], DT)[1].max()) < RAMP_ANGLE
    s2, _ = _fallback_solver(False)
    s2.assign_initial_conditions()
    s2.iterate()
    assert np.array_equal(s2.fields.bathymetry_2d.dat.data_ro, want[-1])


def test_host_fallback_with_a_sediment_field_adds_the_slide():
    """water at rest: nothing erodes, the suspended load leaves the bed alone and the slide alone moves it, as in the run without
    a sediment field"""
    beds = []
    for with_sediment in (True, False):
        s, mesh = _fallback_solver(with_sediment)
        s.assign_initial_conditions()
        if with_sediment:
            assert s.timestepper.tracers['sediment_2d'].host_sediment
        s.iterate()
        beds.append(s.fields.bathymetry_2d.dat.data_ro.copy())
    assert np.array_equal(*beds)
