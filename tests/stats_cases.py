"""Shared builders of the field-statistics tests (tests/test_field_stats.py on the CPU, tests/test_gpu_field_stats.py on the GPU): the
20 x 13 two-marker meshes of the extent of tests/tide_cases.py (so that its bathymetry, tables and solver set-up apply), seeded
states, and the host replay of the accumulator formulas - written here a second time, independent of thetis_amd/fieldstats.py."""
import numpy as np

from thetis_amd.mesh import Mesh2d, _grid_cells, _grid_quads
from tide_cases import LX, LY

EPS = float(np.finfo(np.float64).eps)
NX, NY = 20, 13
M2, S2, K1 = 1.405189e-4, 1.454441e-4, 7.292117e-5
N_FIXED = 8


def stats_mesh(kind='triangles'):
    """'triangles': 20 x 13 quads cut into 520 triangles (3 planes of stride 768: three 256-lane workgroups per node, the last with
    8 cells); 'quads': 260 parallelograms (sheared rectangles; stride 512, the second workgroup with 4 cells); 'general': 260
    convex quadrilaterals that are no parallelograms.  Marker 1: the open end x = 0 before the shear, marker 2: every other side."""
    xs, ys = np.linspace(0.0, LX, NX + 1), np.linspace(0.0, LY, NY + 1)
    xx, yy = np.meshgrid(xs, ys, indexing='ij')
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    left = np.abs(xy[:, 0]) < 1e-6
    if kind == 'general':
        inner = (xy[:, 0] > 1.0) & (xy[:, 0] < LX - 1.0) & (xy[:, 1] > 1.0) & (xy[:, 1] < LY - 1.0)
        xy[:, 0] += np.where(inner, 60.0*np.sin(xy[:, 1]/700.0 + xy[:, 0]/900.0), 0.0)
        xy[:, 1] += np.where(inner, 50.0*np.cos(xy[:, 0]/600.0), 0.0)
    if kind == 'quads':
        xy[:, 0] += 0.1*xy[:, 1]
    cells = _grid_cells(NX, NY, 'left') if kind == 'triangles' else _grid_quads(NX, NY)
    on_left = set(np.nonzero(left)[0].tolist())

    def marker_fn(xm, ym):
        # facet midpoints: on the (sheared) left side exactly where x = 0.1*y for 'quads', x = 0 otherwise
        x0 = xm - (0.1*ym if kind == 'quads' else 0.0)
        return np.where(np.abs(x0) < 1e-6, 1, 2)
    mesh = Mesh2d(xy, cells, marker_fn=marker_fn)
    assert mesh.boundary_markers == [1, 2] and mesh.affine == (kind != 'general') and len(on_left) == NY + 1
    assert mesh.num_cells == (520 if kind == 'triangles' else 260)
    return mesh


def bathymetry(mesh, dry=False):
    """the bathymetry of tests/test_gpu_tide.py; ``dry``: raised so that part of the domain falls dry (wetting-drying)"""
    x, y = mesh.vertex_xy.T
    return 12.0 - 3.0*x/LX + 0.5*np.sin(y/900.0) - (11.5 if dry else 0.0)


def random_state(mesh, seed=3):
    rng = np.random.default_rng(seed)
    n, k = mesh.cells.shape
    uv = 0.05*rng.normal(size=(n, k, 2))
    eta = 0.1*np.cos(np.pi*mesh.cell_xy()[:, :, 0]/LX) + 0.01*rng.normal(size=(n, k))
    return uv, eta


def omegas_for(K, seed=0):
    rng = np.random.default_rng(200 + seed)
    return np.concatenate([[M2, S2, K1], rng.uniform(0.3e-4, 3e-4, size=max(K - 3, 0))])[:K]


def weights_at(omegas, t):
    """cos(omega_0 t), sin(omega_0 t), cos(omega_1 t), ...: numpy, from the product omega*t in double"""
    arg = np.asarray(omegas, dtype=np.float64)*float(t)
    return np.stack([np.cos(arg), np.sin(arg)], axis=1).reshape(-1)


def empty_accumulators(shape, K):
    acc = np.zeros((N_FIXED + 2*K,) + tuple(shape))
    acc[0] = np.inf
    acc[1] = -np.inf
    acc[2] = -np.inf
    return acc


def replay_sample(acc, uv, eta, weights):
    """one sample by the formulas of the issue, every operation a separate numpy call (numpy fuses nothing), left to right"""
    u, v, e = uv[..., 0], uv[..., 1], eta
    uu = np.multiply(u, u)
    vv = np.multiply(v, v)
    q = np.add(uu, vv)
    s = np.sqrt(q)
    acc[0] = np.where(e < acc[0], e, acc[0])
    acc[1] = np.where(e > acc[1], e, acc[1])
    acc[2] = np.where(q > acc[2], q, acc[2])
    acc[3] = np.add(acc[3], e)
    acc[4] = np.add(acc[4], u)
    acc[5] = np.add(acc[5], v)
    acc[6] = np.add(acc[6], s)
    acc[7] = np.add(acc[7], np.multiply(q, s))
    for k in range((acc.shape[0] - N_FIXED)//2):
        acc[N_FIXED + 2*k] = np.add(acc[N_FIXED + 2*k], np.multiply(e, weights[2*k]))
        acc[N_FIXED + 2*k + 1] = np.add(acc[N_FIXED + 2*k + 1], np.multiply(e, weights[2*k + 1]))
    return acc


EXACT = [0, 1, 2, 3, 4, 5]          # e_min, e_max, q_max, e_sum, u_sum, v_sum: +, * and comparisons only (and every C_k, S_k)
SQRT = [6, 7]                       # s_sum, s3_sum: through the device's sqrt


def compare(got, want, n_samples, label=''):
    """bitwise equality of everything built from +, * and comparisons; |device - host| <= (n + 3) eps host for s_sum and s3_sum (a
    one-ulp difference in s gives at most 3 eps on the term q*s, and each of the n additions rounds partial sums of positive terms
    that differ by at most eps times the sum).  Returns the largest measured |device - host| / (eps host) of the two."""
    assert got.shape == want.shape
    exact = EXACT + list(range(N_FIXED, got.shape[0]))
    for j in exact:
        assert np.array_equal(got[j], want[j]), '{:} accumulator {:d}: max |diff| = {:.3e}'.format(
            label, j, float(np.nanmax(np.abs(got[j] - want[j]))))
    worst = 0.0
    for j in SQRT:
        err = np.abs(got[j] - want[j])
        bound = (n_samples + 3)*EPS*want[j]
        worst = max(worst, float((err/(EPS*np.maximum(want[j], 1e-300))).max()))
        assert (err <= bound).all(), '{:} accumulator {:d}: {:.3g} eps'.format(label, j, worst)
    return worst
