"""The bedload pass on the device (swe_bedload_kernel, csrc/swe2d_sediment.hip) against thetis_amd/sediment_model.py's HostSediment:
the q_b planes to the rounding of the two math libraries; the contribution planes and the Exner update bit for bit from the device's
own q_b planes, with and without a sediment field; batches against the step-by-step loop; the solver surface."""
import numpy as np
import pytest

from bedload_cases import ALPHA_SECC, BETA, SURBETA2, SWITCHES, bedload_margin, bedload_state, cell_gradient
from sediment_cases import D50, KS, NU, mesh_case
from thetis_amd.device import Swe2dDevice
from thetis_amd.sediment_model import (HostSediment, bedload_constants, bedload_device_parameters, device_parameters,
                                       sediment_constants)

pytestmark = pytest.mark.gpu

# Largest difference of q_b between the device's math library and numpy, relative to max |q_b|, measured on the MI355X over the
# channel (eight switch combinations), coast and 5000-triangle meshes with the states of bedload_cases.bedload_state:
# 0 on the channel, 2.2e-16 on the coast, 2.5e-16 on the 5000 triangles.
# Asserted: ten times the largest, and never more than the cap of 1e-12 that tells a wrong formula from rounding.
MEASURED_QB = 2.5e-16
QB_BOUND = min(10*MEASURED_QB, 1e-12)
DT = 0.05


def _constants(mag=True, ang=True, sec=True, morfac=1.0):
    return bedload_constants(sediment_constants(D50, KS, NU, morfac=morfac), BETA, SURBETA2, ALPHA_SECC, mag, ang, sec)


def _setup(name, c, with_sediment=False, reorder='auto', seed=1, smooth=False, open_markers=(), solve_exner=False):
    mesh = mesh_case(name)
    bath, uv, eta = bedload_state(mesh, seed=seed, smooth=smooth)
    dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len, reorder=reorder)
    tid = None
    if with_sediment:
        tid = dev.add_tracer()
        dev.sediment_set(tid, device_parameters(c, False, solve_exner))
    dev.bedload_set(bedload_device_parameters(c, solve_exner), open_markers)
    dev.set_state(uv, eta)
    return mesh, bath, uv, eta, dev, tid


def _host_like_device(dev, c):
    """HostSediment in the device's numbering, the device's facet codes (minus the marker slot), and the maps caller -> device of
    nodal and vertex arrays, device -> caller of vertex arrays"""
    cells, xy, nbr = dev._keep[0], dev._keep[1], dev._keep[2]
    host = HostSediment(cells, xy, c)
    nodal = (lambda a: a[dev.perm]) if dev.perm is not None else (lambda a: a)
    vert = (lambda b: b[dev._vperm]) if dev._vperm is not None else (lambda b: b)

    def back(b):
        if dev._vperm is None:
            return b
        out = np.empty_like(b)
        out[dev._vperm] = b
        return out
    return host, nbr, nodal, vert, back


def _check_planes(name, switches):
    c = _constants(*switches)
    mesh, bath, uv, eta, dev, _ = _setup(name, c)
    dev.bedload_update()
    qx, qy, _ = dev.bedload_read()
    want = HostSediment(mesh.cells, mesh.vertex_xy, c).bedload(uv, eta, bath)
    hx, hy = cell_gradient(mesh, bath[mesh.cells])
    ex, ey = cell_gradient(mesh, eta)
    col = lambda g: g[:, None] + 0*eta
    assert bedload_margin(uv[..., 0], uv[..., 1], eta + bath[mesh.cells], col(hx), col(hy), col(ex), col(ey)).min() > 1e-9
    got = np.stack([qx, qy], axis=2)
    assert np.isfinite(got).all() and (want != 0).any() and (want == 0).any()
    assert np.array_equal(got == 0, want == 0)                                   # zeros coincide exactly
    worst = np.abs(got - want).max()/np.abs(want).max()
    print('bedload planes {:} {:}: largest difference {:.3e} of max |q_b|'.format(name, switches, worst))
    dev.close()
    return worst


@pytest.mark.parametrize('switches', SWITCHES)
def test_planes_against_the_replay_on_the_channel(switches):
    assert _check_planes('channel', switches) <= QB_BOUND


@pytest.mark.parametrize('name', ['coast', 'large'])
def test_planes_against_the_replay(name):
    assert _check_planes(name, (True, True, True)) <= QB_BOUND


@pytest.mark.parametrize('name,with_sediment,reorder,opened', [
    ('v63', False, None, True), ('v64', True, 'auto', False), ('v65', False, 'auto', True), ('jack', True, None, True),
    ('large', False, 'auto', False), ('large', True, None, True), ('channel', True, 'auto', True), ('coast', False, None, True)])
def test_contributions_and_exner_bit_for_bit(name, with_sediment, reorder, opened):
    """from the device's own q_b planes: the contribution planes and the bed update of HostSediment in the device's cell and vertex
    order, bit for bit; one marker open (or none), with and without a sediment field"""
    c = _constants(morfac=2000.0)
    mesh = mesh_case(name)
    markers = list(mesh.boundary_markers)
    open_markers = markers[:1] if opened else []
    mesh, bath, uv, eta, dev, tid = _setup(name, c, with_sediment=with_sediment, reorder=reorder, smooth=True, open_markers=open_markers)
    dev.bedload_update()
    qx, qy, contrib = dev.bedload_read()
    hd, nbr, nodal, vert, back = _host_like_device(dev, c)
    mask = sum(1 << dev._slot(m) for m in open_markers)
    want_c = hd.bedload_contributions(np.stack([nodal(qx), nodal(qy)], axis=2), nbr, mask)
    assert np.array_equal(nodal(contrib), want_c) and np.abs(want_c).max() > 0
    if opened:
        closed_c = hd.bedload_contributions(np.stack([nodal(qx), nodal(qy)], axis=2), nbr, 0)
        assert (closed_c != want_c).any()                                        # (the boundary integral is there)
    E = D = S = None
    if with_sediment:
        dev.sediment_update()
        E, D, eq = dev.sediment_read()
        S = 0.5*eq
        dev.tracer_set_state(tid, S)
        E, D, S = nodal(E), nodal(D), nodal(S)
    want = back(hd.exner(E, D, S, nodal(eta), vert(bath), DT, bedload=want_c))
    dev.exner_step()
    got = dev.get_bathymetry()
    assert np.array_equal(got, want) and (got != bath).sum() > len(bath)//2
    assert dev.exner_skipped() == hd.n_skipped
    if with_sediment:                                                            # (the bedload did change the update)
        assert (want != back(hd.exner(E, D, S, nodal(eta), vert(bath), DT))).any()
    dev.close()


def _trench_device(c, with_sediment, bedload, solve_exner=True):
    mesh = mesh_case('channel')
    x = mesh.vertex_xy[:, 0]
    bath = 0.4 + 0.15*np.exp(-((x - 8.0)/2.0)**2)
    n = mesh.num_cells
    uv = np.zeros((n, 3, 2))
    uv[..., 0] = 0.5*0.4/bath[mesh.cells]
    eta = 0.002*np.cos(mesh.vertex_xy[mesh.cells][..., 0]/3.0)
    dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len)
    tid = None
    if with_sediment:
        tid = dev.add_tracer()
        dev.sediment_set(tid, device_parameters(c, False, solve_exner))
        dev.tracer_set_options(False, 1.0, 1.0)
        dev.sediment_set_equilibrium_bc(1)
        dev.tracer_set_state(tid, np.zeros((n, 3)))
    if bedload:
        dev.bedload_set(bedload_device_parameters(c, solve_exner), [1, 2])
    dev.set_bc(1, {'uv': (0.5, 0.0)})
    dev.set_bc(2, {'elev': 0.0})
    dev.set_state(uv, eta)
    return mesh, bath, dev, tid


def _result(dev, tid):
    return dev.get_state() + ((dev.tracer_get_state(tid),) if tid is not None else ()) + (dev.get_bathymetry(),)


@pytest.mark.parametrize('with_sediment,limiter', [(True, True), (True, False), (False, False)])
def test_batches_equal_the_step_by_step_loop(with_sediment, limiter):
    """8 steps in one call against the loop of single launches: state, sediment and bed bit for bit.  A flow-only handle with bedload
    takes swe2d_advance."""
    c = _constants(morfac=300.0)
    out = []
    for batched in (True, False):
        mesh, bath, dev, tid = _trench_device(c, with_sediment, True)
        assert not dev.flow_supported()                                          # never the multi-step dataflow kernel
        if batched and with_sediment:
            dev.advance_coupled(8, tracer_only=False, use_limiter=limiter)
        elif batched:
            dev.advance(8)
        else:
            for _ in range(8):
                for i in range(3):
                    dev.solve_stage(i)
                if with_sediment:
                    dev.sediment_update()
                    for i in range(3):
                        dev.tracer_solve_stage(tid, i)
                    if limiter:
                        dev.tracer_limit(tid)
                dev.bedload_update()
                dev.exner_step()
        res = _result(dev, tid)
        assert all(np.isfinite(a).all() for a in res) and np.abs(res[-1] - bath).max() > 0
        out.append(res)
        dev.close()
    assert all(np.array_equal(p, q) for p, q in zip(*out))
    if not with_sediment:                                                        # advance_coupled orders a flow-only handle the same way
        mesh, bath, dev, tid = _trench_device(c, False, True)
        dev.advance_coupled(8, tracer_only=False, use_limiter=False)
        assert all(np.array_equal(p, q) for p, q in zip(_result(dev, None), out[0]))
        dev.close()


def test_after_bedload_clear_the_update_is_that_of_a_handle_without():
    c = _constants(morfac=300.0)
    res = []
    for had_bedload in (True, False):
        mesh, bath, dev, tid = _trench_device(c, True, had_bedload)
        if had_bedload:
            dev.bedload_update()
            assert np.abs(dev.bedload_read()[0]).max() > 0
            dev.bedload_clear()
        dev.advance_coupled(4, tracer_only=False, use_limiter=True)
        res.append(_result(dev, tid))
        dev.close()
    assert all(np.array_equal(p, q) for p, q in zip(*res)) and np.abs(res[0][-1] - bath).max() > 0
    mesh, bath, dev, tid = _trench_device(c, True, True)
    dev.advance_coupled(4, tracer_only=False, use_limiter=True)
    assert (dev.get_bathymetry() != res[0][-1]).any()                            # (with bedload the bed moves differently)
    dev.close()


@pytest.mark.parametrize('switches', [(True, True, False), (True, True, True), (False, False, False)])
def test_fused_with_the_coefficient_pass_gives_the_same_bits(switches):
    """fuse_with_sediment: the sediment update's launch writes E, D, equilibrium AND q_b with its contributions; planes after one
    update and state, sediment and bed after a batch equal those of the two separate launches bit for bit"""
    c = bedload_constants(sediment_constants(D50, KS, NU, morfac=300.0), BETA, SURBETA2, ALPHA_SECC, *switches)
    res = []
    for fuse in (0, 1):
        mesh, bath, dev, tid = _trench_device(c, True, False)
        dev.bedload_set(dict(bedload_device_parameters(c, True), fuse_with_sediment=fuse), [1, 2])
        dev.sediment_update()
        if not fuse:
            dev.bedload_update()
        planes = dev.sediment_read() + dev.bedload_read()
        dev.advance_coupled(6, tracer_only=False, use_limiter=True)
        res.append(planes + _result(dev, tid) + dev.bedload_read())
        dev.close()
    assert all(np.array_equal(p, q) for p, q in zip(*res)) and np.abs(res[0][3]).max() > 0 and np.abs(res[0][-1]).max() > 0


def test_plan_and_table_ownership():
    """a bedload handle never gets the dataflow plan; the Exner tables outlive whichever of the two models is cleared first"""
    c = _constants(morfac=100.0)
    mesh = mesh_case('large')
    bath, uv, eta = bedload_state(mesh, seed=5, smooth=True)
    dev = Swe2dDevice(mesh, bath, 1e-3, boundary_len=mesh.boundary_len)
    assert dev.flow_supported()
    dev.bedload_set(bedload_device_parameters(c, False))
    assert not dev.flow_supported()
    dev.bedload_clear()
    assert dev.flow_supported()
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(c, False, False))
    dev.bedload_set(bedload_device_parameters(c, True))
    dev.set_state(uv, eta)
    dev.sediment_clear()                                                         # bedload-only from here on
    dev.bedload_update()
    qx, qy, contrib = dev.bedload_read()
    dev.exner_step()
    moved = dev.get_bathymetry()
    hd, nbr, nodal, vert, back = _host_like_device(dev, c)
    want = back(hd.exner(None, None, None, nodal(eta), vert(bath), 1e-3, bedload=nodal(contrib)))
    assert np.array_equal(moved, want) and np.abs(moved - bath).max() > 0 and dev.exner_skipped() == hd.n_skipped
    dev.close()


def _solver(nx=24, ny=4):
    from thetis_amd import options as o
    from thetis_amd.function import Function, get_functionspace
    from thetis_amd.mesh import RectangleMesh
    from thetis_amd.solver2d import FlowSolver2d
    mesh = RectangleMesh(nx, ny, 16.0, 1.1)
    P1 = get_functionspace(mesh, 'CG', 1)
    x = mesh.vertex_xy[:, 0]
    bath = Function(P1, name='bathymetry_2d').assign(0.4 + 0.15*np.exp(-((x - 8.0)/2.0)**2))
    s = FlowSolver2d(mesh, bath)
    m, so = s.options, s.options.sediment_model_options
    so.solve_suspended_sediment = so.solve_exner = so.use_bedload = True
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    so.morphological_acceleration_factor = o.Constant(300.0)
    so.morphological_viscosity = o.Constant(NU)
    m.horizontal_viscosity = None
    m.no_exports = True
    m.set_timestepper_type('SSPRK33')
    for t in (m.swe_timestepper_options, m.tracer_timestepper_options, so.sediment_timestepper_options):
        t.use_automatic_timestep = False
    m.timestep = 0.02
    m.simulation_export_time = 100*0.02
    m.simulation_end_time = 6*0.02
    s.bnd_functions['shallow_water'] = {1: {'flux': o.Constant(-0.22)}, 2: {'elev': o.Constant(0.0)}}
    s.bnd_functions['sediment'] = {1: {'equilibrium': None}, 2: {}}
    uv = Function(get_functionspace(mesh, 'DG', 1, vector=True))
    uv.dat.data[:, 0] = 0.5
    return s, uv


def test_solver_surface_on_the_trench():
    """FlowSolver2d with suspended load and bedload (192 triangles): iterate() equals the generator taken step by step, bit for bit;
    get_bedload_term() is the device's planes; the open markers are those of the shallow-water boundary dict"""
    res = []
    for stepwise in (False, True):
        s, uv = _solver()
        s.assign_initial_conditions(uv=uv)
        assert s.sediment_model.on_device and sorted(s.sediment_model.open_markers()) == [1, 2]
        if stepwise:
            n = sum(1 for _ in s.create_iterator())
            assert n == 6
        else:
            s.iterate()
        dev = s.timestepper.device
        u = s.fields.uv_2d.dat.data_ro[:, 0]
        assert np.isfinite(u).all() and 0.2 < u.min() and u.max() < 0.8
        qbx, qby = s.sediment_model.get_bedload_term()
        rx, ry, _ = dev.bedload_read()
        assert np.array_equal(qbx, rx) and np.array_equal(qby, ry) and qbx.max() > 0
        res.append((s.fields.uv_2d.dat.data_ro.copy(), s.fields.elev_2d.dat.data_ro.copy(), s.fields.sediment_2d.dat.data_ro.copy(),
                    s.fields.bathymetry_2d.dat.data_ro.copy(), qbx.copy()))
    assert all(np.array_equal(p, q) for p, q in zip(*res))
    assert np.abs(res[0][3] - (0.4 + 0.15*np.exp(-((s.mesh2d.vertex_xy[:, 0] - 8.0)/2.0)**2))).max() > 0
