"""Meshes, states and an independent assembly for the Smagorinsky viscosity tests (plain module, no GPU needed)."""
import os

import numpy as np

from thetis_amd.mesh import Mesh2d, RectangleMesh, _rect_marker_fn

COAST = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh')
# (nx, ny) of tests/edge_cases.py around 64 and 256 cells (triangle counts are even: 62 / 64 / 66, 254 / 256 / 258)
EDGE_SIZES = [(31, 1), (8, 4), (11, 3), (127, 1), (16, 8), (43, 3)]
MESH_NAMES = ['two', 'fans', 'coast'] + ['{}x{}'.format(*s) for s in EDGE_SIZES]
_MESHES = {}


def perturbed_grid(nx=4, ny=3, seed=1):
    """a small irregular triangulation: the interior vertices of an nx x ny grid moved by up to a fifth of a cell"""
    m = RectangleMesh(nx, ny, float(nx), float(ny))
    xy = np.array(m.vertex_xy)
    rng = np.random.default_rng(seed)
    inner = (xy[:, 0] > 1e-9) & (xy[:, 0] < nx - 1e-9) & (xy[:, 1] > 1e-9) & (xy[:, 1] < ny - 1e-9)
    xy[inner] += 0.2*rng.uniform(-1, 1, size=(int(inner.sum()), 2))
    return Mesh2d(xy, m.cells, marker_fn=_rect_marker_fn(float(nx), float(ny)))


def two_triangles():
    """one interior facet, every cell with two boundary facets"""
    xy = np.array([[0.0, 0.0], [1.3, 0.1], [1.1, 0.9], [-0.1, 1.2]])
    return Mesh2d(xy, np.array([[0, 1, 2], [0, 2, 3]]))


def fans():
    """a fan of 9 triangles around the interior vertex 0, and 3 more that make a fan of 5 around the boundary vertex 1"""
    ang = np.deg2rad([0.0, 40.0, 75.0, 120.0, 160.0, 200.0, 245.0, 290.0, 320.0])
    rad = np.array([1.0, 1.1, 0.9, 1.0, 1.2, 0.95, 1.05, 1.0, 1.1])
    ring = np.stack([rad*np.cos(ang), rad*np.sin(ang)], axis=1)
    oa = np.deg2rad([-40.0, 0.0, 40.0])
    outer = np.stack([2.0*np.cos(oa), 2.0*np.sin(oa)], axis=1)
    xy = np.concatenate([[[0.05, -0.03]], ring, outer])
    cells = [[0, 1 + j, 1 + (j + 1) % 9] for j in range(9)]
    cells += [[9, 10, 1], [1, 10, 11], [1, 11, 12]]
    return Mesh2d(xy, np.array(cells))


def mesh(name):
    if name not in _MESHES:
        if name == 'two':
            _MESHES[name] = two_triangles()
        elif name == 'fans':
            _MESHES[name] = fans()
        elif name == 'coast':
            from thetis_amd.meshio import read_gmsh
            _MESHES[name] = read_gmsh(COAST)
        elif name == 'grid':
            _MESHES[name] = perturbed_grid()
        else:
            nx, ny = (int(v) for v in name.split('x'))
            _MESHES[name] = RectangleMesh(nx, ny, 2e3*nx, 2e3*ny)
    return _MESHES[name]


def random_velocity(m, seed=0, amp=0.5):
    """a discontinuous P1DG velocity (N, 3, 2)"""
    return amp*np.random.default_rng(100 + seed).normal(size=(m.num_cells, 3, 2))


def lumped(m, cell_values_at_nodes):
    """sum over the (cell, node) pairs of a vertex / sum of A/3, written with np.add.at (independent of the module's table)"""
    num, den = np.zeros(m.num_vertices), np.zeros(m.num_vertices)
    area = m.cell_areas()
    for i in range(3):
        np.add.at(num, m.cells[:, i], cell_values_at_nodes[:, i])
        np.add.at(den, m.cells[:, i], area/3.0)
    return num/den


# ---- the weak gradient assembled on its own: generic Gauss rules, physical coordinates, a dense solve per cell
def _bary(p, x):
    """barycentric coordinates of the points x (Q, 2) in the triangle p (3, 2)"""
    T = np.array([[p[0, 0] - p[2, 0], p[1, 0] - p[2, 0]], [p[0, 1] - p[2, 1], p[1, 1] - p[2, 1]]])
    l01 = np.linalg.solve(T, (x - p[2]).T).T
    return np.concatenate([l01, 1.0 - l01.sum(axis=1, keepdims=True)], axis=1)


def independent_weak_gradient(m, uv):
    """(N, 2, 2, 3): M g = -int d_x phi_i u_c + sum_f int_f u_hat phi_i n_x, u_hat the mean of the traces (own trace on the boundary)"""
    from thetis_amd.function import farm_quadrature
    phi_c, w_c = farm_quadrature(3, 4)                        # a cell rule of degree 4, weights sum to 1
    gx, gw = np.polynomial.legendre.leggauss(3)               # a facet rule of degree 5 on [-1, 1]
    s, ws = 0.5*(gx + 1.0), 0.5*gw
    xy, cells, nbr = np.asarray(m.vertex_xy), np.asarray(m.cells), np.asarray(m.cell_nbr)
    G = np.zeros((m.num_cells, 2, 2, 3))
    for k in range(m.num_cells):
        p = xy[cells[k]]
        xq = phi_c @ p
        lam = _bary(p, xq)
        e1, e2 = p[1] - p[0], p[2] - p[0]
        area = 0.5*abs(e1[0]*e2[1] - e1[1]*e2[0])
        M = area*np.einsum('q,qi,qj->ij', w_c, lam, lam)
        # gradients of the barycentric coordinates from the inverse of [p; 1]
        B = np.linalg.inv(np.column_stack([p, np.ones(3)]))   # rows 0, 1: d lambda_i / dx, d lambda_i / dy
        for c in range(2):
            uq = lam @ uv[k, :, c]
            for d in range(2):
                rhs = -area*B[d]*np.dot(w_c, uq)
                for f in range(3):
                    a, b = p[f], p[(f + 1) % 3]
                    t = b - a
                    length = np.hypot(*t)
                    n = np.array([t[1], -t[0]])/length
                    if np.dot(n, p[(f + 2) % 3] - a) > 0:     # outward: away from the opposite vertex
                        n = -n
                    xf = a[None, :] + s[:, None]*t[None, :]
                    lf = _bary(p, xf)
                    mine = lf @ uv[k, :, c]
                    if nbr[k, f] >= 0:
                        kn = nbr[k, f]
                        other = _bary(xy[cells[kn]], xf) @ uv[kn, :, c]
                        hat = 0.5*(mine + other)
                    else:
                        hat = mine
                    rhs = rhs + length*n[d]*np.einsum('q,q,qi->i', ws, hat, lf)
                G[k, c, d] = np.linalg.solve(M, rhs)
    return G
