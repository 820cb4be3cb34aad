"""CPU tests of the section transports (thetis_amd/sections.py): the host geometry, the numpy restatement of the device's sums
against closed forms, the callback through FlowSolver2d on the host stand-in device, the refusals and the ABI names."""
import ctypes
import os
import types

import numpy as np
import pytest

import section_cases as sc
from cpu_device import CpuSwe2dDevice
from thetis_amd import Constant, RectangleMesh, SectionTransportCallback, _lib, callback, read_gmsh, sections, solver2d
from thetis_amd.pointeval import PointLocator
from tide_cases import make_solver, tide_mesh

COAST = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh')


def _rect():
    return RectangleMesh(6, 4, 6.0, 4.0)


def _inside_length(mesh, pts):
    """the covered length of a polyline, independently of the cutter: every segment is cut at the EXTERIOR facets alone
    (``cell_nbr < 0``), between two such crossings it is inside or outside as a whole, which its midpoint tells"""
    pts = np.asarray(pts, dtype=np.float64)
    P = mesh.cell_xy()
    k = P.shape[1]
    c, f = np.nonzero(np.asarray(mesh.cell_nbr) < 0)
    a, e = P[c, f], P[c, (f + 1) % k] - P[c, f]
    cross = lambda u, v: u[..., 0]*v[..., 1] - u[..., 1]*v[..., 0]
    total = 0.0
    for p, q in zip(pts[:-1], pts[1:]):
        d = q - p
        den = cross(d, e)
        assert (np.abs(den) > 1e-9*np.hypot(*d)*np.hypot(*e.T)).all()   # (the test's lines run along no exterior facet)
        t, s = cross(a - p, e)/den, cross(a - p, d)/den
        t = np.unique(np.concatenate([[0.0, 1.0], t[(s >= 0.0) & (s <= 1.0) & (t > 0.0) & (t < 1.0)]]))
        mid = 0.5*(t[1:] + t[:-1])
        inside = PointLocator(mesh, p + mid[:, None]*d).cells >= 0
        total += float(np.sum((t[1:] - t[:-1])[inside]))*np.hypot(*d)
    return total


# line, mesh, covered length (None: by brute force, to 1e-3 relative only)
RECT_LINES = {
    'oblique': ([(0.3, 0.2), (5.5, 3.7)], np.hypot(5.2, 3.5)),
    'interior vertex': ([(0.3, 0.2), (2.4, 1.3), (2.9, 3.8)], np.hypot(2.1, 1.1) + np.hypot(0.5, 2.5)),
    'vertices and edges': ([(0.0, 0.0), (3.0, 3.0), (3.0, 1.0), (5.0, 1.0)], np.hypot(3.0, 3.0) + 2.0 + 2.0),
    'leaves and re-enters': ([(-1.0, 2.5), (2.5, 2.5), (2.5, 5.0), (4.5, 5.0), (4.5, 0.5)], 2.5 + 1.5 + 3.5),
}


def _check_pieces(mesh, p, covered, rel):
    P = mesh.cell_xy()
    assert abs(p.total_length - covered) <= rel*covered, (p.total_length, covered)
    assert np.abs(p.weights.sum(axis=2) - 1.0).max() <= 1e-12 and p.weights.min() >= -1e-12
    mid = 0.5*(p.start + p.end)
    ok, _ = PointLocator._reference_coordinates(P[p.cell], mid, 1e-12)
    assert ok.all()                                                    # the midpoint of every piece lies in its cell
    assert (p.length > 0.0).all() and np.allclose(np.hypot(*(p.end - p.start).T), p.length, rtol=1e-12, atol=1e-12*np.abs(P).max())
    keys = set((int(c),) + tuple(np.round(m, 9)) for c, m in zip(p.cell, mid))
    assert len(keys) == len(p)                                         # no duplicates
    assert np.allclose(np.hypot(*p.normal.T), 0.5*p.length, rtol=1e-12, atol=0.0)
    # both Gauss points lie on the piece, symmetric about its midpoint
    g = np.einsum('pqi,pij->pqj', p.weights, P[p.cell])
    assert np.allclose(0.5*(g[:, 0] + g[:, 1]), mid, rtol=0.0, atol=1e-9*np.abs(P).max())


@pytest.mark.parametrize('line', sorted(RECT_LINES))
def test_cut_polyline_on_the_rectangle(line):
    pts, covered = RECT_LINES[line]
    mesh = _rect()
    p = sections.cut_polyline(mesh, pts)
    _check_pieces(mesh, p, covered, 1e-12)


def test_a_piece_along_a_mesh_edge_belongs_to_the_cell_of_its_midpoint():
    mesh = _rect()
    p = sections.cut_polyline(mesh, [(3.0, 1.0), (3.0, 3.0)])
    assert len(p) == 2
    want = PointLocator(mesh, [(3.0, 1.5), (3.0, 2.5)], tolerance=sections.CUT_TOLERANCE).cells
    assert np.array_equal(p.cell, want)
    again = sections.cut_polyline(mesh, [(3.0, 1.0), (3.0, 3.0)])
    assert np.array_equal(again.cell, p.cell) and np.array_equal(again.weights, p.weights)


def test_cut_polyline_on_the_coast_mesh():
    mesh = read_gmsh(COAST)
    xy = mesh.vertex_xy
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    c = 0.5*(lo + hi)
    v0, v1 = xy[mesh.cells[100, 0]], xy[mesh.cells[100, 1]]          # through two vertices, i.e. along an edge, and beyond
    lines = {
        'oblique': [lo + 0.13*(hi - lo), lo + (0.81, 0.77)*(hi - lo)],
        'interior vertex': [lo + 0.2*(hi - lo), c + 0.013*(hi - lo), lo + (0.7, 0.3)*(hi - lo)],
        'vertices and edges': [v0 - 3.0*(v1 - v0), v0, v1, v1 + 2.5*(v1 - v0)],
        'leaves and re-enters': [lo - 0.1*(hi - lo), c, hi + 0.1*(hi - lo), (hi[0] + 1.0, lo[1] - 1.0), c],
    }
    scale = np.abs(xy).max()
    for name, pts in lines.items():
        p = sections.cut_polyline(mesh, pts)
        covered = _inside_length(mesh, pts)
        assert 0.3*sum(np.hypot(*(np.subtract(b, a))) for a, b in zip(pts[:-1], pts[1:])) < covered
        _check_pieces(mesh, p, covered, 1e-12)
        # the pieces tile what they cover: consecutive pieces share their end points, or the first ends and the next begins on the
        # outline of the mesh - a step of 1e-7 of the domain further along the one, back along the other, is outside
        gap = np.hypot(*(p.start[1:] - p.end[:-1]).T)
        far = np.nonzero(gap >= 1e-9*scale)[0]
        direction = (p.end - p.start)/p.length[:, None]
        beyond = np.concatenate([p.end[far] + 1e-7*scale*direction[far], p.start[far + 1] - 1e-7*scale*direction[far + 1]])
        assert (PointLocator(mesh, beyond).cells < 0).all(), name
        if name == 'leaves and re-enters':
            assert len(far) >= 1


def test_a_section_without_pieces_and_quadrilaterals_are_refused():
    mesh = _rect()
    with pytest.raises(ValueError, match='no piece'):
        sections.cut_polyline(mesh, [(-3.0, -1.0), (-1.0, -2.0)])
    with pytest.raises(ValueError, match='no piece'):
        sections.boundary_pieces(mesh, 7)
    with pytest.raises(NotImplementedError, match='quadrilateral'):
        sections.cut_polyline(tide_mesh('quads'), [(100.0, 100.0), (5000.0, 3000.0)])
    assert len(sections.boundary_pieces(tide_mesh('general'), 1)) == 4


def _sum_abs(host, pieces, uv, eta, h, tracers=()):
    return np.abs(host.piece_terms(pieces, uv, eta, h, tracers)).sum(axis=1)


@pytest.mark.parametrize('line', sorted(RECT_LINES))
def test_reversing_the_polyline_negates_the_transport(line):
    pts, _ = RECT_LINES[line]
    mesh = _rect()
    uv, eta, bath, tr = sc.random_state(mesh, 5)
    h = bath[mesh.cells]
    fwd, bwd = sections.cut_polyline(mesh, pts), sections.cut_polyline(mesh, pts[::-1])
    host = sections.HostSections([fwd, bwd])
    v, bad = host.eval(uv, eta, h, tr)
    scale = _sum_abs(host, fwd, uv, eta, h, tr)
    assert bad == 0
    assert abs(v[0, 0] + v[1, 0]) <= 1e-13*scale[0]
    assert abs(v[0, 1] - v[1, 1]) <= 1e-13*scale[1]
    for q in (2, 3):
        assert abs(v[0, q] + v[1, q]) <= 1e-13*scale[q]


@pytest.mark.parametrize('nonlinear', [True, False])
def test_closed_forms_on_a_straight_section(nonlinear):
    """uniform u, linear eta and h: Q = len H(mid) u.n and area = len H(mid) - H u.n is linear along the line.  Every term has one
    sign (H > 0, u.n > 0).  1e-13 relative, the bound of the turbine power test: a few hundred terms of one sign, each within a few eps."""
    mesh = RectangleMesh(6, 4, 600.0, 400.0)
    a, b = np.array([30.0, 20.0]), np.array([550.0, 370.0])
    p = sections.cut_polyline(mesh, [a, b])
    xy = mesh.vertex_xy[mesh.cells]
    eta = 0.3 + 1e-3*xy[..., 0] - 5e-4*xy[..., 1]
    h = 12.0 - 4e-3*xy[..., 0] + 2e-3*xy[..., 1]
    u0 = np.array([0.7, -0.2])
    uv = np.broadcast_to(u0, xy.shape).copy()
    c = 1.5 + 0.0*eta
    v, bad = sections.HostSections([p], nonlinear).eval(uv, eta, h, [c])
    mid, d = 0.5*(a + b), b - a
    length = np.hypot(*d)
    n = np.array([d[1], -d[0]])/length
    H = (12.0 - 4e-3*mid[0] + 2e-3*mid[1]) + ((0.3 + 1e-3*mid[0] - 5e-4*mid[1]) if nonlinear else 0.0)
    assert bad == 0 and u0 @ n > 0
    assert abs(v[0, 0] - length*H*(u0 @ n)) <= 1e-13*length*H*(u0 @ n)
    assert abs(v[0, 1] - length*H) <= 1e-13*length*H
    assert abs(v[0, 2] - 1.5*length*H*(u0 @ n)) <= 1e-13*1.5*length*H*(u0 @ n)
    assert abs(p.total_length - length) <= 1e-12*length


def test_closed_loop_equals_the_divergence_of_its_block():
    """a continuous P1 state and a closed loop of mesh edges, counter-clockwise (right-hand normal = outward): the loop transport is
    the integral of div(H u) over the block, cell by cell A div(H u)(centroid) - H u is quadratic, its divergence linear"""
    mesh = _rect()
    xv = mesh.vertex_xy
    Hv = 10.0 + 0.8*xv[:, 0] - 0.5*xv[:, 1] + 0.05*xv[:, 0]*xv[:, 1]          # any values at the vertices: P1 per cell, continuous
    ev = 0.2*np.sin(xv[:, 0]) + 0.1*xv[:, 1]
    uvv = np.stack([0.5 + 0.1*xv[:, 0]**2 - 0.2*xv[:, 1], -0.3 + 0.15*xv[:, 0]*xv[:, 1]], axis=1)
    cells = mesh.cells
    p = sections.cut_polyline(mesh, [(1.0, 1.0), (4.0, 1.0), (4.0, 3.0), (1.0, 3.0), (1.0, 1.0)])
    host = sections.HostSections([p])
    v, bad = host.eval(uvv[cells], ev[cells], (Hv - ev)[cells])
    P = mesh.cell_xy()
    cen = P.mean(axis=1)
    block = np.nonzero((cen[:, 0] > 1.0) & (cen[:, 0] < 4.0) & (cen[:, 1] > 1.0) & (cen[:, 1] < 3.0))[0]
    assert len(block) == 12
    want = 0.0
    for k in block:
        x, y = P[k, :, 0], P[k, :, 1]
        A2 = (x[1] - x[0])*(y[2] - y[0]) - (x[2] - x[0])*(y[1] - y[0])
        gx = np.array([y[1] - y[2], y[2] - y[0], y[0] - y[1]])/A2          # gradients of the barycentric coordinates
        gy = np.array([x[2] - x[1], x[0] - x[2], x[1] - x[0]])/A2
        Hn, un = Hv[cells[k]], uvv[cells[k]]
        div = (gx @ Hn)*un[:, 0].mean() + (gy @ Hn)*un[:, 1].mean() + Hn.mean()*(gx @ un[:, 0] + gy @ un[:, 1])
        want += 0.5*A2*div
    scale = _sum_abs(host, p, uvv[cells], ev[cells], (Hv - ev)[cells])[0]
    assert bad == 0 and abs(v[0, 0] - want) <= 1e-13*scale, (v[0, 0], want, scale)


def test_limb_split_and_rounding():
    x = np.array([1.0e15 + 0.125, -3.5e-7, 2.0**-160, -(2.0**77), 1.0/3.0])
    limbs, bad = sections.split_limbs(x)
    assert bad == 0 and np.array_equal(limbs, CpuSwe2dDevice._limbs(x))
    assert sections.limbs_to_double(limbs) == CpuSwe2dDevice.limbs_to_double(limbs)
    limbs, bad = sections.split_limbs([np.nan, np.inf, 2.0**78, 1.0])
    assert bad == 3 and sections.limbs_to_double(limbs) == 1.0
    assert sections.fma(0.1, 10.0, -1.0)[()] == 5.551115123125783e-17 and 0.1*10.0 - 1.0 == 0.0


# ---- the callback through FlowSolver2d on the host stand-in device
SECTIONS = {'mid': [(4000.0, -100.0), (4000.0, 2100.0), (4300.0, 4100.0)], 'open': 1}


def _solver(n_steps, n_export, outdir=None):
    return make_solver(tide_mesh('triangles'), Constant(0.2), dt=0.3, n_steps=n_steps, n_export=n_export, tracer=True, outdir=outdir)


@pytest.mark.parametrize('batch', [True, False])
def test_callback_on_the_host_device(ref_so, monkeypatch, tmp_path, batch):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    dt = 0.3
    s = _solver(12, 6, outdir=str(tmp_path))
    cb = SectionTransportCallback(s, SECTIONS, tracers=('tracer_2d',), every=2, name='straits', append_to_log=False)
    s.add_callback(cb, 'timestep')
    if batch:
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == 12
    twin = _solver(12, 6, outdir=str(tmp_path))
    host = sections.HostSections(cb.pieces)
    want_t, want = [], []
    for _ in twin.create_iterator():
        it = twin.iteration + 1                   # (the generator yields before the counters move on)
        if it % 2 == 0:
            f = twin.fields
            v, bad = host.eval(f.uv_2d.cell_node_values(), f.elev_2d.cell_node_values(), f.bathymetry_2d.cell_node_values(),
                               [f.tracer_2d.cell_node_values()])
            assert bad == 0
            want_t.append(it*dt)
            want.append(v)
    want = np.array(want)
    r = cb.result()
    assert np.array_equal(r['time'], np.array(want_t)) and len(want_t) == 6
    assert np.array_equal(r['transport'], want[:, :2, 0]) and np.array_equal(r['area'], want[:, :2, 1])
    assert r['tracer_transport'].shape == (6, 2, 1) and np.array_equal(r['tracer_transport'][..., 0], want[:, :2, 2])
    assert np.isfinite(want[:, :2, :3]).all() and (r['area'] > 0.0).all() and np.abs(r['transport']).min() > 0.0
    assert np.array_equal(r['n_unsummable'], np.zeros(6, dtype=np.int64))
    # the length: 'mid' loses its parts outside the mesh; 'open' is the side x = 0
    assert abs(r['length'][0] - (2100.0 + np.hypot(300.0, 2000.0)*(1900.0/2000.0))) < 1e-9 and abs(r['length'][1] - 4000.0) < 1e-9
    cum = np.zeros((6, 2))
    for i in range(1, 6):
        cum[i] = cum[i - 1] + 0.5*(r['transport'][i] + r['transport'][i - 1])*(r['time'][i] - r['time'][i - 1])
    assert np.array_equal(r['cumulative_volume'], cum)
    assert len(cb.history) == 6 and cb.history[2][0] == want_t[2] and np.array_equal(cb.history[2][1], want[2, :2, 0])
    assert cb.message_str(*cb.history[0][1:]).startswith('straits: mid Q = ')
    d = np.load(os.path.join(str(tmp_path), 'diagnostic_straits.npz'))
    assert np.array_equal(d['transport'], r['transport']) and np.array_equal(d['cumulative_volume'], cum)
    assert list(d['section_names']) == ['mid', 'open'] and list(d['tracer_names']) == ['tracer_2d']
    assert np.array_equal(s.fields.elev_2d.dat.data_ro, twin.fields.elev_2d.dat.data_ro)
    # a call evaluates the state now
    q, a, c = cb()
    assert np.array_equal(q, want[-1, :2, 0]) and np.array_equal(a, want[-1, :2, 1]) and c.shape == (2, 1)


def test_callback_at_exports(ref_so, monkeypatch, tmp_path):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    s = _solver(12, 6, outdir=str(tmp_path))
    cb = SectionTransportCallback(s, {'open': 1}, append_to_log=False, export_to_hdf5=False)
    s.add_callback(cb, 'export')
    s.iterate()
    assert np.allclose(cb.result()['time'], [0.0, 1.8, 3.6]) and not os.path.exists(os.path.join(str(tmp_path), 'diagnostic_sections.npz'))


def test_exported_names():
    assert callback.SectionTransportCallback is sections.SectionTransportCallback is SectionTransportCallback
    assert 'SectionTransportCallback' in callback.__all__
    for name in sc.SYMBOLS:
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 12


def test_abi_of_the_built_library(hip_lib):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sc.SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.swe2d_abi_version() == 12


def test_refusals(ref_so, monkeypatch):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    s = _solver(4, 4)
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_SECTIONS'):
        SectionTransportCallback(s, {'s{:d}'.format(i): 1 for i in range(17)})
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_SECTION_TRACERS'):
        SectionTransportCallback(s, {'open': 1}, tracers=['tracer_2d']*5)
    with pytest.raises(ValueError, match='no piece'):
        SectionTransportCallback(s, {'nowhere': [(-10.0, -10.0), (-20.0, -5.0)]})
    cb = SectionTransportCallback(s, {'open': 1}, append_to_log=False)
    s.comm = types.SimpleNamespace(size=2, rank=0)
    with pytest.raises(NotImplementedError, match='several ranks'):
        cb.evaluate()
    q = make_solver(tide_mesh('quads'), Constant(0.2), n_steps=2)
    with pytest.raises(NotImplementedError, match='quadrilateral'):
        SectionTransportCallback(q, {'mid': [(4000.0, 100.0), (4000.0, 3900.0)]})
    assert len(SectionTransportCallback(q, {'open': 1}).pieces[0]) == 4
    w = _solver(2, 2)
    w.options.use_wetting_and_drying = True
    with pytest.raises(NotImplementedError, match='wetting-drying'):
        SectionTransportCallback(w, {'open': 1})
