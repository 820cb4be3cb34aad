"""The Smagorinsky viscosity's numpy restatement (thetis_amd/smagorinsky.py) on its own: known answers, an independent assembly,
the clip, the refusals, and the host-stepped path of a device class without the closure."""
import types

import numpy as np
import pytest

import smagorinsky_cases as sc
from thetis_amd.cgproject import elem_size_p1
from thetis_amd.mesh import RectangleMesh
from thetis_amd.smagorinsky import MAX_H_DIFF_FACTOR, HostSmagorinsky, check_supported, vertex_cell_table

# about 50 FP64 operations on O(1) data
TOL = 1e-12


def _rel(a, b):
    return float(np.abs(a - b).max()/np.abs(b).max())


def test_continuous_linear_velocity_has_the_known_answer():
    m = sc.mesh('grid')
    a, b, c, d = 0.3, -0.7, 1.1, 0.4
    p = m.cell_xy()
    uv = np.stack([a*p[:, :, 0] + b*p[:, :, 1], c*p[:, :, 0] + d*p[:, :, 1]], axis=2)
    s = HostSmagorinsky(m, 0.17, min_val=0.0, max_viscosity=1e30)
    G = s.weak_gradient(uv)
    want = np.broadcast_to(np.array([[a, b], [c, d]])[None, :, :, None], G.shape)
    print('weak gradient: rel', _rel(G, want))
    assert _rel(G, want) < TOL
    # nu_v = C_s^2 |S| times the lumped projection of h^2, h the P1 element size, integrated here by the rule on its own
    from thetis_amd.function import triangle_quadrature
    bary, w = triangle_quadrature()
    he = elem_size_p1(m)[m.cells]
    hq2 = (he @ bary.T)**2                                              # (N, Q)
    mom = m.cell_areas()[:, None]*np.einsum('q,qi,nq->ni', w, bary, hq2)
    S = np.sqrt((a - d)**2 + (b + c)**2)
    want_nu = 0.17**2*S*sc.lumped(m, mom)
    s.update(uv, 1.0)
    print('nu: rel', _rel(s.nu, want_nu))
    assert _rel(s.nu, want_nu) < TOL
    assert np.array_equal(s.total, s.nu)


@pytest.mark.parametrize('name', ['grid', 'two', 'fans'])
def test_weak_gradient_against_an_independent_assembly(name):
    m = sc.mesh(name)
    uv = sc.random_velocity(m, seed=3)
    nb = (np.asarray(m.cell_nbr) < 0).sum(axis=1)
    assert nb.max() >= 2                                               # a cell with two boundary facets
    if name == 'two':
        assert m.num_cells == 2 and (np.asarray(m.cell_nbr) >= 0).sum() == 2
    got = HostSmagorinsky(m, 0.1).weak_gradient(uv)
    want = sc.independent_weak_gradient(m, uv)
    print(name, 'rel', _rel(got, want))
    assert _rel(got, want) < TOL


def test_vertex_table_lists_every_pair_once_in_ascending_cell_order():
    m = sc.mesh('fans')
    ptr, idx = vertex_cell_table(m.cells, m.num_vertices)
    assert ptr[0] == 0 and ptr[-1] == 3*m.num_cells and sorted(idx.tolist()) == sorted(((np.arange(m.num_cells)[:, None] << 2) | np.arange(3)).ravel().tolist())
    for v in range(m.num_vertices):
        ent = idx[ptr[v]:ptr[v + 1]]
        assert (np.diff(ent >> 2) > 0).all() and (m.cells[ent >> 2, ent & 3] == v).all()
    assert ptr[1] - ptr[0] == 9 and ptr[2] - ptr[1] == 5              # the two fans
    s = HostSmagorinsky(m, 0.1)
    mom = np.random.default_rng(0).uniform(size=(m.num_cells, 3))
    assert _rel(s.lumped_projection(mom), sc.lumped(m, mom)) < TOL


def _clip_case():
    m = RectangleMesh(8, 4, 8e3, 4e3)
    p = m.cell_xy()
    uv = np.zeros((m.num_cells, 3, 2))
    uv[:, :, 0] = 0.4                                                   # uniform flow: no strain
    right = p[:, :, 0].min(axis=1) >= 5e3
    uv[right, :, 1] = 1e-3*(p[right, :, 0] - 5e3)/1e3                   # a weak shear on the right
    jump = int(np.argmin(np.abs(p.mean(axis=1) - np.array([1.5e3, 2e3])).sum(axis=1)))
    uv[jump, :, 0] = 1e4                                                # a strong jump on the left
    return m, uv


def test_clipping_floor_ceiling_and_in_between():
    m, uv = _clip_case()
    dt = 10.0
    s = HostSmagorinsky(m, 0.1)
    assert s.min_val == 1e-10
    he = elem_size_p1(m)
    s.update(uv, dt)
    max_v = he*he/120.0/dt
    assert MAX_H_DIFF_FACTOR == 1.0/120.0 and _rel(s.max_v(dt), max_v) < 1e-15
    at_min, at_max = s.nu == 1e-10, s.nu == s.max_v(dt)
    between = ~at_min & ~at_max
    print('vertices at the floor / the ceiling / between:', at_min.sum(), at_max.sum(), between.sum())
    assert at_min.sum() > 0 and at_max.sum() > 0 and between.sum() > 0
    assert (s.nu >= 1e-10).all() and (s.nu <= s.max_v(dt)).all()
    raw = s.lumped_projection(s.moments)
    assert np.array_equal(s.nu[between], raw[between]) and (raw[at_max] >= s.max_v(dt)[at_max]).all() and (raw[at_min] <= 1e-10).all()
    # another dt: the ceiling follows it
    s.update(uv, 2.5)
    assert np.array_equal(s.nu[at_max], s.max_v(2.5)[at_max]) and _rel(s.max_v(2.5), 4.0*max_v) < 1e-15
    # the override replaces it, whatever dt
    o = HostSmagorinsky(m, 0.1, max_viscosity=0.37)
    o.update(uv, dt)
    assert (o.nu[at_max] == 0.37).all() and o.nu.max() == 0.37
    # the background is added after the clip
    bg = np.linspace(1.0, 2.0, m.num_vertices)
    assert np.array_equal(o.update(uv, dt, bg), bg + o.nu)


def _options(**kw):
    from thetis_amd.options import ModelOptions2d
    o = ModelOptions2d()
    o.use_smagorinsky_viscosity = True
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_options_defaults():
    from thetis_amd.options import ModelOptions2d
    o = ModelOptions2d()
    assert o.use_smagorinsky_viscosity is False and float(o.smagorinsky_coefficient) == 0.1 and o.smagorinsky_max_viscosity is None


def test_refusals_name_the_option():
    tri, quad = RectangleMesh(3, 2, 3.0, 2.0), RectangleMesh(3, 2, 3.0, 2.0, quadrilateral=True)
    check_supported(_options(), tri, 1)
    for args in ((_options(), quad, 1), (_options(use_wetting_and_drying=True), tri, 1), (_options(), tri, 2)):
        with pytest.raises(NotImplementedError, match='use_smagorinsky_viscosity'):
            check_supported(*args)
    with pytest.raises(NotImplementedError, match='use_smagorinsky_viscosity'):
        HostSmagorinsky(quad, 0.1)


@pytest.mark.parametrize('what', ['quadrilaterals', 'wetting_drying', 'ranks'])
def test_solver_refuses_by_name(what):
    from thetis_amd import solver2d
    from thetis_amd.function import Function, get_functionspace
    m = RectangleMesh(3, 2, 3e3, 2e3, quadrilateral=what == 'quadrilaterals')
    s = solver2d.FlowSolver2d(m, Function(get_functionspace(m, 'CG', 1)).assign(10.0))
    s.options.use_smagorinsky_viscosity = True
    if what == 'wetting_drying':
        s.options.use_wetting_and_drying = True
    if what == 'ranks':
        s.comm = types.SimpleNamespace(size=2)
    with pytest.raises(NotImplementedError, match='use_smagorinsky_viscosity'):
        s.create_fields()


def test_host_stepped_path_of_a_device_class_without_the_closure(ref_so):
    """a device class without ``smag_set``: the stepper evaluates HostSmagorinsky on the state read back in front of every step and
    hands the total over as a plain viscosity; iterate() then goes step by step"""
    from cpu_device import CpuSwe2dDevice
    from thetis_amd import solver2d
    from thetis_amd.function import Function, get_functionspace
    from thetis_amd.options import Constant

    class Recording(CpuSwe2dDevice):
        def set_viscosity(self, nu, **kwargs):                          # (the stand-in itself has no viscosity term)
            self.__dict__.setdefault('seen', []).append(None if nu is None else np.array(nu, dtype=float, ndmin=1).copy())

    m = RectangleMesh(6, 3, 6e3, 3e3)
    P1 = get_functionspace(m, 'CG', 1)
    s = solver2d.FlowSolver2d(m, Function(P1).assign(10.0))
    s._device_cls = Recording
    o = s.options
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.timestep = 2.0
    o.simulation_export_time = 6.0
    o.simulation_end_time = 5.0
    o.no_exports = True
    o.use_smagorinsky_viscosity = True
    o.horizontal_viscosity = Constant(0.5)
    P1DGv = get_functionspace(m, 'DG', 1, vector=True)
    uv0 = Function(P1DGv)
    uv0.dat.data[...] = sc.random_velocity(m, seed=5, amp=0.05).reshape(-1, 2)
    s.assign_initial_conditions(uv=uv0)
    ts = s.timestepper
    assert ts.forced_per_stage and not ts._smag_on_device
    host = HostSmagorinsky(m, 0.1)
    first = host.update(sc.random_velocity(m, seed=5, amp=0.05), 2.0, 0.5)
    nu0 = s.fields.smag_visc_2d.dat.data_ro.copy()
    assert np.array_equal(nu0, host.nu) and nu0.max() > 1e-10
    s.iterate()
    seen = [v for v in ts.device.seen if v is not None and v.size == m.num_vertices]
    assert len(seen) == 3 and np.array_equal(seen[0], first)            # one total per step
    assert not np.array_equal(seen[1], seen[0])
