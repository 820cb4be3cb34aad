"""Shared builders of the section-transport tests (tests/test_sections.py on the CPU, tests/test_gpu_sections.py on the GPU): meshes,
seeded P1DG states, the section sets of the bit-for-bit comparisons and the host's sums for them."""
import numpy as np

from thetis_amd import RectangleMesh, _lib, sections
from thetis_amd.mesh import Mesh2d, _grid_quads

SYMBOLS = ('swe2d_sections_set', 'swe2d_sections_clear', 'swe2d_sections_eval_limbs', 'swe2d_sections_eval',
           'swe2d_sections_rows_reserve', 'swe2d_sections_rows_append', 'swe2d_sections_rows_read')


def random_state(mesh, seed, n_tracers=2):
    """uv (N, k, 2), eta (N, k), vertex bathymetry (V,), tracers [(N, k)]: discontinuous, every depth positive"""
    rng = np.random.default_rng(seed)
    n, k = mesh.cells.shape
    uv = rng.uniform(-1.0, 1.0, (n, k, 2))
    eta = rng.uniform(-0.5, 0.5, (n, k))
    bath = rng.uniform(5.0, 15.0, mesh.num_vertices)
    tracers = [rng.uniform(0.0, 2.0, (n, k)) for _ in range(n_tracers)]
    return uv, eta, bath, tracers


def big_mesh():
    """40 x 30 quads cut into 2400 triangles, 400 m x 300 m, markers 1 .. 4 on the four sides"""
    return RectangleMesh(40, 30, 400.0, 300.0)


def big_sections(mesh):
    """the slots of the bit-for-bit test: [diagonal with more pieces than two workgroups hold, one piece, through vertices and along
    edges, boundary marker 1, None (unused), boundary marker 3]"""
    diag = sections.cut_polyline(mesh, [(3.0, 2.0), (397.0, 296.0), (5.0, 290.0)])
    assert len(diag) > 128
    one = sections.cut_polyline(mesh, [(101.0, 52.0), (103.0, 53.0)])
    assert len(one) == 1
    edges = sections.cut_polyline(mesh, [(50.0, 50.0), (120.0, 120.0), (120.0, 200.0), (200.0, 200.0)])
    return [diag, one, edges, sections.boundary_pieces(mesh, 1), None, sections.boundary_pieces(mesh, 3)]


def quad_mesh(general):
    """12 x 9 quadrilaterals, 120 m x 90 m; ``general``: interior vertices moved, so that no cell is a parallelogram; otherwise
    sheared into parallelograms.  Marker 1: x = 0 side, marker 2: the rest."""
    nx, ny = 12, 9
    xs, ys = np.linspace(0.0, 120.0, nx + 1), np.linspace(0.0, 90.0, ny + 1)
    xx, yy = np.meshgrid(xs, ys, indexing='ij')
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    shear = 0.0 if general else 0.3
    if general:
        inner = (xy[:, 0] > 1.0) & (xy[:, 0] < 119.0) & (xy[:, 1] > 1.0) & (xy[:, 1] < 89.0)
        xy[:, 0] += np.where(inner, 2.0*np.sin(xy[:, 1]/7.0 + xy[:, 0]/9.0), 0.0)
        xy[:, 1] += np.where(inner, 1.5*np.cos(xy[:, 0]/6.0), 0.0)
    else:
        xy[:, 0] += shear*xy[:, 1]
    mesh = Mesh2d(xy, _grid_quads(nx, ny), marker_fn=lambda xm, ym: np.where(np.abs(xm - shear*ym) < 1e-6, 1, 2))
    assert mesh.boundary_markers == [1, 2] and mesh.affine == (not general)
    return mesh


def flat(section_list):
    """the arguments of ``Swe2dDevice.sections_set`` for a list of Pieces / None"""
    live = [(s, p) for s, p in enumerate(section_list) if p is not None]
    return (len(section_list), np.concatenate([np.full(len(p), s) for s, p in live]), np.concatenate([p.cell for _, p in live]),
            np.concatenate([p.weights for _, p in live]), np.concatenate([p.normal for _, p in live]))


def host_limbs(mesh, section_list, uv, eta, bath, tracers, nonlinear=True):
    return sections.HostSections(section_list, nonlinear).eval_limbs(uv, eta, np.asarray(bath)[mesh.cells], tracers)


def values_of(limbs):
    out = np.zeros(limbs.shape[:2])
    for s in range(limbs.shape[0]):
        for q in range(limbs.shape[1]):
            out[s, q] = sections.limbs_to_double(limbs[s, q])
    return out


assert _lib.SECTION_VALUES == 6 and _lib.MAX_SECTIONS == 16
