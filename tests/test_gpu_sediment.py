"""The sediment passes on the device (csrc/swe2d_sediment.hip) against thetis_amd/sediment_model.py's HostSediment: the coefficient
planes to the rounding of the two math libraries; source planes, 'equilibrium' facets and the Exner update bit for bit from the
device's own planes; swe2d_advance_coupled batches against the step-by-step loop; the closed forms of the relaxation and of the
equilibrium fixed point; neighbours unchanged."""
import numpy as np
import pytest

from sediment_cases import D50, KS, NU, branch_state, mesh_case, threshold_margin
from thetis_amd import _lib
from thetis_amd.device import Swe2dDevice
from thetis_amd.sediment_model import HostSediment, device_parameters, sediment_constants

pytestmark = pytest.mark.gpu

# Largest relative difference of E, D and equilibrium between the device's math library and numpy, measured on the MI355X over the
# channel, coast and 5000-triangle meshes with the states of sediment_cases.branch_state: 4.1e-16, 1.6e-14 and
# 8.5e-15.  Asserted: ten times the largest, and never more than the cap of 1e-12 that tells a wrong formula from rounding.
MEASURED_PLANES = 1.6e-14
PLANES_BOUND = min(10*MEASURED_PLANES, 1e-12)
DT = 0.05


def _setup(name, conservative=False, solve_exner=False, reorder='auto', seed=1, smooth=False, morfac=1.0, dt=DT):
    mesh = mesh_case(name)
    bath, uv, eta = branch_state(mesh, seed=seed, smooth=smooth)
    c = sediment_constants(D50, KS, NU, morfac=morfac)
    dev = Swe2dDevice(mesh, bath, dt, boundary_len=mesh.boundary_len, reorder=reorder)
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(c, conservative, solve_exner))
    dev.set_state(uv, eta)
    return mesh, bath, uv, eta, c, dev, tid


def _host_like_device(mesh, dev, c, conservative):
    """HostSediment in the device's numbering (the Exner gather sums a vertex's cells in ascending DEVICE order) and the maps
    caller -> device of nodal and vertex arrays, device -> caller of vertex arrays"""
    cells, xy = dev._keep[0], dev._keep[1]
    host = HostSediment(cells, xy, c, conservative=conservative)
    nodal = (lambda a: a[dev.perm]) if dev.perm is not None else (lambda a: a)
    vert = (lambda b: b[dev._vperm]) if dev._vperm is not None else (lambda b: b)

    def back(b):
        if dev._vperm is None:
            return b
        out = np.empty_like(b)
        out[dev._vperm] = b
        return out
    return host, nodal, vert, back


def _rel(a, b):
    return np.abs(a - b)/np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize('name', ['channel', 'coast', 'large'])
def test_planes_against_the_replay(name):
    mesh, bath, uv, eta, c, dev, tid = _setup(name)
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    hE, hD, heq = HostSediment(mesh.cells, mesh.vertex_xy, c).coefficients(uv, eta, bath)
    H = eta + bath[mesh.cells]
    assert threshold_margin(uv[..., 0], uv[..., 1], H).min() > 1e-9          # no node where a select could differ
    assert np.isfinite(E).all() and np.isfinite(D).all() and (hE > 0).any() and (hE == 0).any()
    assert np.array_equal(E == 0, hE == 0)
    worst = max(_rel(E, hE)[hE > 0].max(), _rel(D, hD).max(), _rel(eq, heq)[heq > 0].max())
    print('sediment planes {:}: largest relative difference {:.3e}'.format(name, worst))
    assert worst <= PLANES_BOUND
    dev.close()


@pytest.mark.parametrize('name,conservative,reorder', [('channel', False, None), ('channel', True, 'auto'), ('coast', False, 'auto'),
                                                       ('coast', True, None)])
def test_source_exner_and_facets_bit_for_bit(name, conservative, reorder):
    mesh, bath, uv, eta, c, dev, tid = _setup(name, conservative=conservative, reorder=reorder, smooth=True, morfac=200.0)
    markers = list(mesh.boundary_markers)
    dev.sediment_set_equilibrium_bc(markers[0])
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    host = HostSediment(mesh.cells, mesh.vertex_xy, c, conservative=conservative)
    H = host.depth(eta, bath)
    S0 = 1.5*eq*(H if conservative else 1.0)*(1.0 + 0.2*np.cos(np.arange(eq.size).reshape(eq.shape)))
    dev.tracer_set_state(tid, S0)
    # the per-facet table on the 'equilibrium' marker, untouched elsewhere
    tab = dev.sediment_read_bc()
    slot = dev._slot(markers[0])
    cells, facets = dev.boundary_facets(slot)
    assert len(cells) > 0 and np.array_equal(tab[cells, facets], host.boundary_values(eq, eta, bath)[cells])
    mask = np.ones(tab.shape[:2], dtype=bool)
    mask[cells, facets] = False
    assert not tab[mask].any()
    # the source planes of every stage from that stage's input buffer
    for i in range(3):
        dev.tracer_solve_stage(tid, i)
        S_in = dev.tracer_get_buffer(tid, i)
        assert np.array_equal(dev.tracer_get_source(tid), host.source(E, D, S_in, eta, bath)), 'stage {:d}'.format(i)
    # the Exner update, in the device's own vertex and cell order
    S1 = dev.tracer_get_state(tid)
    hd, nodal, vert, back = _host_like_device(mesh, dev, c, conservative)
    want = back(hd.exner(nodal(E), nodal(D), nodal(S1), nodal(eta), vert(bath), DT))
    assert np.array_equal(dev.get_bathymetry(), bath)
    dev.exner_step()
    got = dev.get_bathymetry()
    assert np.array_equal(got, want) and np.abs(got - bath).max() > 0 and dev.exner_skipped() == hd.n_skipped == 0
    # ForwardEuler takes the same source pass
    dev.tracer_forward_euler(tid)
    assert np.array_equal(dev.tracer_get_source(tid), host.source(E, D, S1, eta, got))
    dev.close()


@pytest.mark.parametrize('name', ['v63', 'v64', 'v65', 'jack', 'large'])
def test_exner_vertex_list_shapes(name):
    """63, 64 and 65 vertices (the tail of a wave), a vertex of valence 8, and more than one workgroup of vertices"""
    mesh, bath, uv, eta, c, dev, tid = _setup(name, solve_exner=True, smooth=True, morfac=500.0)
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    S = 0.5*eq
    dev.tracer_set_state(tid, S)
    hd, nodal, vert, back = _host_like_device(mesh, dev, c, False)
    want = back(hd.exner(nodal(E), nodal(D), nodal(S), nodal(eta), vert(bath), DT))
    dev.exner_step()
    got = dev.get_bathymetry()
    assert np.array_equal(got, want) and (got != bath).sum() > len(bath)//2
    dev.close()


def test_exner_floor_on_the_device():
    """still water full of sediment: the bed rises, but not at the vertex under 0.5 mm of water nor at the two that share a cell with
    it alone (below the reference level a the deposition coefficient is 1e12 ws: their update would bury them); they are counted"""
    mesh = mesh_case('channel')
    bath = np.full(mesh.vertex_xy.shape[0], 0.5)
    eta = np.zeros((mesh.num_cells, 3))
    eta[mesh.cells == 0] = -0.4995
    uv = np.zeros((mesh.num_cells, 3, 2))
    c = sediment_constants(D50, KS, NU, morfac=100.0)
    dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len)
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(c, False, True))
    dev.set_state(uv, eta)
    S = np.full((mesh.num_cells, 3), 1e-3)
    dev.tracer_set_state(tid, S)
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    assert not E.any()
    dev.exner_step()
    got = dev.get_bathymetry()
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    want = host.exner(E, D, S, eta, bath, DT)
    kept = want == bath
    assert kept[0] and 1 <= host.n_skipped == kept.sum() < len(bath)//2 and (want[~kept] < bath[~kept]).all() and (want > 0.4).all()
    assert dev.exner_skipped() == host.n_skipped and np.array_equal(got == bath, kept)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    dev.close()


def _step_by_step(dev, tid, n, limiter, plain=None, tracer_only=False):
    for _ in range(n):
        if not tracer_only:
            for i in range(3):
                dev.solve_stage(i)
        if plain is not None:
            for i in range(3):
                dev.tracer_solve_stage(plain, i)
            if limiter:
                dev.tracer_limit(plain)
        dev.sediment_update()
        for i in range(3):
            dev.tracer_solve_stage(tid, i)
        if limiter:
            dev.tracer_limit(tid)
        dev.exner_step()


@pytest.mark.parametrize('limiter,diffusion,conservative', [(True, False, False), (False, False, True), (True, True, False)])
def test_batches_equal_the_step_by_step_loop(limiter, diffusion, conservative):
    """12 steps of swe2d_advance_coupled in one call against the loop of single launches: state, sediment and bathymetry bit for bit;
    a handle rebuilt from the read-back bathymetry and state continues bit for bit (the flow sees the moved bed)"""
    out = []
    for batched in (True, False):
        mesh = mesh_case('channel')
        x = mesh.vertex_xy[:, 0]
        bath = 0.4 + 0.15*np.exp(-((x - 8.0)/2.0)**2)                      # the trench
        n = mesh.num_cells
        uv = np.zeros((n, 3, 2))
        uv[..., 0] = 0.5*0.4/bath[mesh.cells]
        eta = 0.002*np.cos(mesh.vertex_xy[mesh.cells][..., 0]/3.0)
        c = sediment_constants(D50, KS, NU, morfac=300.0)
        dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len)
        tid = dev.add_tracer()
        dev.sediment_set(tid, device_parameters(c, conservative, True))
        dev.tracer_set_options(False, 1.0, 1.0)
        if diffusion:
            dev.tracer_set_diffusivity(tid, 0.01, 1.0)
        dev.set_bc(1, {'uv': (0.5, 0.0)})
        dev.set_bc(2, {'elev': 0.0})
        dev.sediment_set_equilibrium_bc(1)
        dev.set_state(uv, eta)
        dev.tracer_set_state(tid, np.zeros((n, 3)))
        if batched:
            dev.advance_coupled(12, tracer_only=False, use_limiter=limiter)
        else:
            _step_by_step(dev, tid, 12, limiter)
        res = dev.get_state() + (dev.tracer_get_state(tid), dev.get_bathymetry())
        assert all(np.isfinite(a).all() for a in res) and np.abs(res[3] - bath).max() > 0 and res[2].max() > 0
        if batched:
            # a new handle from what was read back: three more steps on both
            dev2 = Swe2dDevice(mesh, res[3], DT, boundary_len=mesh.boundary_len)
            t2 = dev2.add_tracer()
            dev2.sediment_set(t2, device_parameters(c, conservative, True))
            dev2.tracer_set_options(False, 1.0, 1.0)
            if diffusion:
                dev2.tracer_set_diffusivity(t2, 0.01, 1.0)
            dev2.set_bc(1, {'uv': (0.5, 0.0)})
            dev2.set_bc(2, {'elev': 0.0})
            dev2.sediment_set_equilibrium_bc(1)
            dev2.set_state(res[0], res[1])
            dev2.tracer_set_state(t2, res[2])
            for d in (dev, dev2):
                d.advance_coupled(3, tracer_only=False, use_limiter=limiter)
            a = dev.get_state() + (dev.tracer_get_state(tid), dev.get_bathymetry())
            b = dev2.get_state() + (dev2.tracer_get_state(t2), dev2.get_bathymetry())
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
            dev2.close()
        out.append(res)
        dev.close()
    for p, q, what in zip(out[0], out[1], ('uv', 'eta', 'sediment', 'bathymetry')):
        assert np.array_equal(p, q), what


def test_relaxation_closed_form():
    """tracer_only, uniform flow and depth, S0 = 0, SSPRK33: every node follows S_{n+1} = S_eq + (S_n - S_eq) P(z), z = -D dt/H,
    P = 1 + z + z^2/2 + z^3/6, for 10 steps, on the closed 4 x 3 mesh (no boundary condition set).  Measured on the MI355X: 1.9e-16
    of S_eq."""
    mesh = mesh_case('small')
    n = mesh.num_cells
    bath = np.full(mesh.vertex_xy.shape[0], 0.397)
    uv = np.zeros((n, 3, 2))
    uv[..., 0] = 0.5
    c = sediment_constants(D50, KS, NU)
    dt = 0.2
    dev = Swe2dDevice(mesh, bath, dt, boundary_len=mesh.boundary_len)
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(c, False, False))
    dev.tracer_set_options(False, 1.0, 1.0)
    dev.set_state(uv, np.zeros((n, 3)))
    dev.tracer_set_state(tid, np.zeros((n, 3)))
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    assert np.ptp(E) == 0 and np.ptp(D) == 0
    s_eq, z = float(eq[0, 0]), -float(D[0, 0])*dt/0.397
    P = 1 + z + z*z/2 + z**3/6
    S = 0.0
    worst = 0.0
    for _ in range(10):
        dev.advance_coupled(1, tracer_only=True, use_limiter=False)
        S = s_eq + (S - s_eq)*P
        worst = max(worst, np.abs(dev.tracer_get_state(tid) - S).max()/s_eq)
    print('relaxation: largest deviation from the closed form relative to S_eq {:.3e}'.format(worst))
    assert worst <= 1e-13 + PLANES_BOUND
    dev.close()


def test_equilibrium_is_a_fixed_point():
    """S = S_eq everywhere, uniform flow through the channel with 'equilibrium' at the inflow and an open outflow, tracer_only,
    solve_exner, 5 steps: S stays, the bed does not move"""
    mesh = mesh_case('small')
    n = mesh.num_cells
    bath = np.full(mesh.vertex_xy.shape[0], 0.397)
    uv = np.zeros((n, 3, 2))
    uv[..., 0] = 0.5
    c = sediment_constants(D50, KS, NU, morfac=100.0)
    dt = 0.2
    dev = Swe2dDevice(mesh, bath, dt, boundary_len=mesh.boundary_len)
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(c, False, True))
    dev.tracer_set_options(False, 1.0, 1.0)
    dev.sediment_set_equilibrium_bc(1)
    dev.set_state(uv, np.zeros((n, 3)))
    dev.sediment_update()
    E, D, eq = dev.sediment_read()
    dev.tracer_set_state(tid, eq)
    dev.advance_coupled(5, tracer_only=True, use_limiter=True)
    S = dev.tracer_get_state(tid)
    drift = np.abs(S - eq).max()/eq.max()
    moved = np.abs(dev.get_bathymetry() - bath).max()
    print('fixed point: S drift {:.3e} relative, bed moved {:.3e} (bound {:.3e})'.format(drift, moved, 5*dt*c['fac']*E.max()*1e-12))
    assert drift <= 1e-13 + PLANES_BOUND
    assert moved <= 5*dt*c['fac']*float(E.max())*1e-12
    dev.close()


def test_plain_tracer_next_to_a_sediment_field_is_unchanged():
    """a plain tracer gives the same bits with and without a sediment field on the handle (no Exner: the flow is the same)"""
    res = []
    for with_sediment in (False, True):
        mesh = mesh_case('channel')
        bath, uv, eta = branch_state(mesh, seed=4, smooth=True)
        dev = Swe2dDevice(mesh, bath, 0.01, boundary_len=mesh.boundary_len)
        plain = dev.add_tracer()
        dev.tracer_set_options(False, 1.0, 1.0)
        xc = mesh.vertex_xy[mesh.cells]
        dev.tracer_set_state(plain, 1.0 + 0.5*np.sin(xc[..., 0]))
        if with_sediment:
            tid = dev.add_tracer()
            dev.sediment_set(tid, device_parameters(sediment_constants(D50, KS, NU), False, False))
        dev.set_state(0.1*uv, eta)
        dev.advance_coupled(4, tracer_only=False, use_limiter=True)
        res.append(dev.get_state() + (dev.tracer_get_state(plain),))
        if with_sediment:
            assert dev.tracer_get_state(tid).max() > 0                     # (the sediment field did step)
        dev.close()
    assert all(np.array_equal(p, q) for p, q in zip(*res))


def test_only_solve_exner_takes_the_dataflow_kernel_away():
    """what the step plan covers, by swe2d_flow_supported: a handle with solve_exner is not stepped by the multi-step dataflow kernel;
    a sediment field without Exner, and the handle after swe2d_sediment_clear, keep it.  Which path each size and option takes
    without sediment is pinned by tests/test_gpu_step_plan.py, which this change leaves passing."""
    mesh = mesh_case('large')
    bath, uv, eta = branch_state(mesh, seed=5, smooth=True)
    dev = Swe2dDevice(mesh, bath, 1e-3, boundary_len=mesh.boundary_len)
    assert dev.flow_supported()
    tid = dev.add_tracer()
    dev.sediment_set(tid, device_parameters(sediment_constants(D50, KS, NU), False, False))
    assert dev.flow_supported()
    dev.sediment_set(tid, device_parameters(sediment_constants(D50, KS, NU), False, True))
    assert not dev.flow_supported()
    dev.sediment_clear()
    assert dev.flow_supported()
    with pytest.raises(_lib.Swe2dError, match='no sediment model'):
        dev.sediment_update()
    dev.close()
