"""The Smagorinsky viscosity on the device (csrc/swe2d_smag.hip): the two kernels against the numpy restatement bit for bit, the seam
in the advance calls against a run that makes the update on the host, and a handle without the closure."""
import numpy as np
import pytest

import smagorinsky_cases as sc
from thetis_amd import _lib
from thetis_amd.cgproject import elem_size_p1
from thetis_amd.device import Swe2dDevice
from thetis_amd.smagorinsky import HostSmagorinsky

pytestmark = pytest.mark.gpu
DT, CS = 0.3, 0.15


def _bath(mesh):
    x, y = mesh.vertex_xy.T
    return 12.0 + 0.5*np.sin(x/(1.0 + np.abs(x).max())) + 0.3*np.cos(y/(1.0 + np.abs(y).max()))


def _background(mesh):
    return 0.5 + 0.5*np.random.default_rng(11).uniform(size=mesh.num_vertices)


def _eta(mesh, seed=0):
    return 0.05*np.random.default_rng(200 + seed).normal(size=(mesh.num_cells, 3))


def _device(mesh, background=True, dt=DT):
    dev = Swe2dDevice(mesh, _bath(mesh), dt, boundary_len=mesh.boundary_len)
    if background:
        dev.set_viscosity(_background(mesh), sipg_factor=1.5)
    return dev


def _report(what, got, want):
    d = np.abs(got - want).max()
    print('{:10s} max |device - host| = {:.3e} (rel {:.3e})'.format(what, d, d/max(np.abs(want).max(), 1e-300)))


# ---- 5. kernels against the restatement
@pytest.mark.parametrize('name', sc.MESH_NAMES)
def test_kernels_against_the_restatement_bit_for_bit(hip_lib, name):
    mesh = sc.mesh(name)
    he = elem_size_p1(mesh)
    uv = sc.random_velocity(mesh, seed=1)
    # a scale at which some vertices reach the ceiling h^2/(120 dt) and others do not
    scale = 0.5*np.median(he)/DT
    uv = uv*scale
    dev = _device(mesh)
    dev.set_state(uv, _eta(mesh))
    dev.smag_set(CS, he)
    host = HostSmagorinsky(mesh, CS, h_elem=he)
    bg = _background(mesh)
    host.update(uv, DT, bg)
    got = {w: dev.smag_read(w) for w in ('gradient', 'moments', 'nu', 'total')}
    want = {'gradient': host.grad, 'moments': host.moments, 'nu': host.nu, 'total': host.total}
    for w in got:
        _report(w, got[w], want[w])
    for w in got:
        assert got[w].shape == want[w].shape and np.array_equal(got[w], want[w]), w
    at_max = host.nu == host.max_v(DT)
    print(name, 'vertices at the ceiling', int(at_max.sum()), 'of', mesh.num_vertices)
    # the update twice on the same state: identical bits
    dev.smag_update()
    dev.smag_update()
    for w in ('moments', 'nu', 'total'):
        assert np.array_equal(dev.smag_read(w), got[w]), w
    # another dt needs no upload: the vertex pass reads it
    dev.set_dt(4.0*DT)
    dev.smag_update()
    host.update(uv, 4.0*DT, bg)
    assert np.array_equal(dev.smag_read('nu'), host.nu) and np.array_equal(dev.smag_read('total'), host.total)
    # the override and another floor; a constant background
    dev.set_viscosity(0.25, sipg_factor=1.5)
    cap = float(np.median(host.nu))
    dev.smag_set(CS, he, min_val=1e-6, max_viscosity=cap)
    o = HostSmagorinsky(mesh, CS, h_elem=he, min_val=1e-6, max_viscosity=cap)
    o.update(uv, 4.0*DT, 0.25)
    assert np.array_equal(dev.smag_read('nu'), o.nu) and np.array_equal(dev.smag_read('total'), o.total)
    assert o.nu.max() == cap
    dev.close()


def test_device_numbering_does_not_change_the_sums(hip_lib):
    """the lumped projection adds a vertex's cells in the caller's ascending order whatever the device numbering"""
    mesh = sc.mesh('coast')
    he = elem_size_p1(mesh)
    uv = sc.random_velocity(mesh, seed=2)
    out = []
    for reorder in ('auto', None, np.random.default_rng(3).permutation(mesh.num_cells)):
        dev = Swe2dDevice(mesh, _bath(mesh), DT, boundary_len=mesh.boundary_len, reorder=reorder)
        dev.set_state(uv, _eta(mesh))
        dev.smag_set(CS, he)
        out.append(dev.smag_read('total'))
        dev.close()
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_refusals_by_message(hip_lib):
    from thetis_amd.mesh import RectangleMesh
    quad = RectangleMesh(4, 3, 4e3, 3e3, quadrilateral=True)
    dev = Swe2dDevice(quad, np.full(quad.num_vertices, 10.0), DT)
    ptr = np.zeros(quad.num_vertices + 1, dtype=np.int32)
    idx = np.zeros(4*quad.num_cells, dtype=np.int32)
    he = np.ones(quad.num_vertices)
    rc = dev.lib.swe2d_smag_set(dev.h, 0.1, he.ctypes.data_as(_lib._dp), 1e-10, -1.0, ptr.ctypes.data_as(_lib._ip), idx.ctypes.data_as(_lib._ip))
    assert rc == _lib.ERR_UNSUPPORTED and b'quadrilaterals' in dev.lib.swe2d_last_error(dev.h)
    dev.close()
    mesh = sc.mesh('8x4')
    dev = Swe2dDevice(mesh, _bath(mesh) - 11.5, DT)
    dev.set_wetting_and_drying(0.5)
    with pytest.raises(_lib.Swe2dError, match='wetting-drying'):
        dev.smag_set(CS, elem_size_p1(mesh))
    dev.close()
    dev = Swe2dDevice(mesh, _bath(mesh), DT, n_owned=mesh.num_cells - 4, boundary_len=mesh.boundary_len)
    with pytest.raises(_lib.Swe2dError, match='partitions'):
        dev.smag_set(CS, elem_size_p1(mesh))
    dev.close()
    dev = _device(mesh)
    with pytest.raises(_lib.Swe2dError, match='swe2d_smag_set'):
        dev.smag_update()
    dev.close()


# ---- 6. the seam
def _solver(mesh, smag, stepper='SSPRK33', tracer=False, n_steps=6, nu=None):
    from thetis_amd import solver2d
    from thetis_amd.function import Function, get_functionspace
    from thetis_amd.options import Constant
    P1 = get_functionspace(mesh, 'CG', 1)
    s = solver2d.FlowSolver2d(mesh, Function(P1).assign(_bath(mesh)))
    o = s.options
    o.swe_timestepper_type = stepper
    o.swe_timestepper_options.use_automatic_timestep = False
    o.timestep = DT
    o.simulation_export_time = n_steps*DT
    o.simulation_end_time = (n_steps - 0.5)*DT
    o.no_exports = True
    o.manning_drag_coefficient = Constant(0.02)
    o.sipg_factor = Constant(1.5)
    o.horizontal_viscosity = nu if nu is not None else Function(P1).assign(_background(mesh))
    if smag is not None:
        o.use_smagorinsky_viscosity = smag
        o.smagorinsky_coefficient = Constant(CS)
    if tracer:
        o.add_tracer_2d('tracer_2d', 'Depth averaged tracer', 'Tracer2d', source=None, diffusivity=None)
        o.tracer_timestepper_type = stepper
        o.tracer_timestepper_options.use_automatic_timestep = False
    s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.05)}, 2: {'un': Constant(0.01)}}
    uv0 = Function(get_functionspace(mesh, 'DG', 1, vector=True))
    uv0.dat.data[...] = sc.random_velocity(mesh, seed=4, amp=0.5).reshape(-1, 2)
    kw = {'tracer': Function(P1).interpolate(lambda x, y: 1.0 + (x > 0.5*mesh.lx))} if tracer else {}
    s.assign_initial_conditions(elev=Function(P1).interpolate(lambda x, y: 0.05*np.cos(np.pi*x/mesh.lx)), uv=uv0, **kw)
    return s


def _final(s, tracer):
    out = [s.fields.uv_2d.dat.data_ro.copy(), s.fields.elev_2d.dat.data_ro.copy()]
    if tracer:
        out.append(s.fields.tracer_2d.dat.data_ro.copy())
    return out


@pytest.mark.parametrize('case', ['ssprk33', 'forward_euler', 'tracer'])
def test_iterate_equals_the_host_made_update_step_by_step(hip_lib, case):
    from thetis_amd import coupled_timeintegrator_2d, rungekutta
    from thetis_amd.function import Function, get_functionspace
    stepper = 'ForwardEuler' if case == 'forward_euler' else 'SSPRK33'
    tracer = case == 'tracer'
    mesh = sc.mesh('16x8')
    n_steps = 6
    cls = (coupled_timeintegrator_2d.GeneralCoupledTimeIntegrator2D if tracer
           else (rungekutta.ForwardEuler if case == 'forward_euler' else rungekutta.SSPRK33))
    calls, orig = [], cls.advance_steps

    def counting(self, t, n, **kw):
        calls.append(n)
        return orig(self, t, n, **kw)
    cls.advance_steps = counting
    try:
        a = _solver(mesh, True, stepper, tracer, n_steps)
        assert a.timestepper.__class__ is cls and not a.timestepper.forced_per_stage
        a.iterate()
    finally:
        cls.advance_steps = orig
    assert calls == [n_steps]                                            # iterate() stayed batched: one call into the library
    got = _final(a, tracer)
    nu_end = a.fields.smag_visc_2d.dat.data_ro.copy()

    # the run in which the test makes the update: the restatement on the state read back, the total as a plain viscosity Function
    P1 = get_functionspace(mesh, 'CG', 1)
    nu_f = Function(P1).assign(_background(mesh))
    b = _solver(mesh, None, stepper, tracer, n_steps, nu=nu_f)
    host = HostSmagorinsky(mesh, CS)
    bg = _background(mesh)
    for k in range(n_steps):
        uv = b.fields.uv_2d.dat.data_ro.reshape(mesh.num_cells, 3, 2)
        nu_f.assign(host.update(uv, DT, bg))
        b.timestepper.advance(k*DT, update_forcings=lambda t: None)
    want = _final(b, tracer)
    for g, w, what in zip(got, want, ('uv', 'elev', 'tracer')):
        _report(what, g, w)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[0], b.fields.uv_2d.dat.data_ro*0)
    # the exported field: the closure viscosity of the state that is there
    host.update(want[0].reshape(mesh.num_cells, 3, 2), DT, bg)
    assert np.array_equal(nu_end, host.nu) and nu_end.max() > 1e-10


# ---- 7. off is off
@pytest.mark.parametrize('background', [True, False])
def test_a_handle_without_the_closure_is_what_it_was(hip_lib, background):
    mesh = sc.mesh('16x8')
    uv, eta = 0.05*sc.random_velocity(mesh, seed=6), _eta(mesh)
    res = []
    for mode in ('never', 'cleared', 'on'):
        dev = _device(mesh, background)
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
        if mode != 'never':
            dev.set_state(uv*3.0, eta)
            dev.smag_set(CS, elem_size_p1(mesh))
            dev.advance(2)
        if mode == 'cleared':
            dev.smag_clear()
        dev.set_state(uv, eta)
        dev.advance(6)
        res.append(dev.get_state())
        dev.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][0], res[2][0])                      # (and the closure, left on, does change the run)


def test_the_option_false_is_the_default_run(hip_lib):
    mesh = sc.mesh('16x8')
    runs = []
    for smag in (None, False):
        s = _solver(mesh, smag)
        assert not hasattr(s.fields, 'smag_visc_2d') and not s.timestepper._smag_on_device
        s.iterate()
        runs.append(_final(s, False))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
