"""Shared helpers of the particle-tracking tests (tests/test_particles.py on the CPU, tests/test_gpu_particles.py on the GPU): an
independent replay of the tracker's algorithm - one particle at a time in plain Python floats (IEEE double, nothing fused), written
from the specification and not imported from thetis_amd/particles.py -, seeded particle clouds, and the closed forms of the tests.

The algorithm, per ACTIVE particle at x in cell k and one move of dt_move:

    u1 = U(x, k);  (xm, km) = probe(x, k, (0.5*dt_move)*u1);  u2 = U(xm, km);  (x', k') = move(x, k, dt_move*u2)

U: barycentric interpolation of the cell's nodal velocities; move: the straight walk from cell to cell through the facet with the
smallest crossing parameter, ending inside a cell, at an open boundary (EXITED), at a wall (shortened by 2^-10 of the way to it) or,
after 64 cells, nowhere (LOST, position unchanged); probe: the same walk, whose open boundaries and walls only end it.
"""
import math

import numpy as np

ACTIVE, EXITED, LOST = 0, 1, 2
MAX_HOPS = 64
ARRIVED, EXIT, WALL, NOWHERE = 'arrived', 'exit', 'wall', 'nowhere'


def _div(a, b):
    """a/b as IEEE double division (Python raises where the divisor is zero)"""
    if b != 0.0:
        return a/b
    with np.errstate(all='ignore'):
        return float(np.float64(a)/np.float64(b))


class Replay(object):
    """the particle set of the replay on a mesh given by ``cells`` (N, 3), ``vertex_xy`` (V, 2), ``cell_nbr`` (N, 3; a boundary
    facet: -marker) and ``cell_nbr_facet`` (N, 3)"""

    def __init__(self, mesh, xy, particle_cells):
        self.cv = np.asarray(mesh.cells).tolist()
        self.vxy = np.asarray(mesh.vertex_xy, dtype=np.float64).tolist()
        self.nbr = np.asarray(mesh.cell_nbr).tolist()
        self.nbf = np.asarray(mesh.cell_nbr_facet).tolist()
        self.xy = np.array(xy, dtype=np.float64).reshape(-1, 2)
        n = len(self.xy)
        self.cells = np.array(particle_cells, dtype=np.int32).reshape(n)
        self.status = np.zeros(n, dtype=np.int32)
        self.markers = np.zeros(n, dtype=np.int32)
        self.hits = np.zeros(n, dtype=np.int32)
        self.most_cells = 0                         # the most cells one walk visited, over all advances so far

    def facet_coordinates(self, k, px, py):
        """(m_0, m_1, m_2): m_f vanishes on facet f, which joins the local vertices f and f + 1"""
        p0, p1, p2 = (self.vxy[v] for v in self.cv[k])
        ax, ay = p1[0] - p0[0], p1[1] - p0[1]
        bx, by = p2[0] - p0[0], p2[1] - p0[1]
        det = ax*by - bx*ay
        dx, dy = px - p0[0], py - p0[1]
        l1 = _div(dx*by - bx*dy, det)
        l2 = _div(ax*dy - dx*ay, det)
        l0 = (1.0 - l1) - l2
        return l2, l0, l1

    def velocity(self, uv, k, px, py):
        l2, l0, l1 = self.facet_coordinates(k, px, py)
        w = uv[k]
        return ((l0*w[0][0] + l1*w[1][0]) + l2*w[2][0], (l0*w[0][1] + l1*w[1][1]) + l2*w[2][1])

    def walk(self, x, y, k, dx, dy, open_markers):
        tx, ty = x + dx, y + dy
        entered = -1
        for hop in range(MAX_HOPS):
            self.most_cells = max(self.most_cells, hop + 1)
            mx = self.facet_coordinates(k, x, y)
            my = self.facet_coordinates(k, tx, ty)
            best, s_best = -1, 0.0
            for f in range(3):
                if f != entered and my[f] < 0.0:
                    s = _div(mx[f], mx[f] - my[f])
                    if best < 0 or s < s_best:
                        best, s_best = f, s
            if best < 0:
                return ARRIVED, tx, ty, k, 0
            code = self.nbr[k][best]
            if code >= 0:
                entered, k = self.nbf[k][best], code
                continue
            if -code in open_markers:
                return EXIT, x + s_best*dx, y + s_best*dy, k, -code
            f = s_best*(1.0 - 2.0**-10)
            return WALL, x + f*dx, y + f*dy, k, -code
        return NOWHERE, x, y, k, 0

    def advance(self, uv, dt_move, open_markers=()):
        """one move of every ACTIVE particle in the nodal velocities ``uv`` (N, 3, 2) as ``get_state`` returns them"""
        uv = np.asarray(uv, dtype=np.float64).tolist()
        dt_move = float(dt_move)
        open_markers = set(int(m) for m in open_markers)
        for p in range(len(self.xy)):
            if self.status[p] != ACTIVE:
                continue
            x, y, k = float(self.xy[p, 0]), float(self.xy[p, 1]), int(self.cells[p])
            u, v = self.velocity(uv, k, x, y)
            half = 0.5*dt_move
            how, xm, ym, km, _ = self.walk(x, y, k, half*u, half*v, open_markers)
            if how != NOWHERE:
                u, v = self.velocity(uv, km, xm, ym)
                how, xn, yn, kn, marker = self.walk(x, y, k, dt_move*u, dt_move*v, open_markers)
            if how == NOWHERE:
                self.status[p] = LOST
                continue
            self.xy[p], self.cells[p] = (xn, yn), kn
            if how == EXIT:
                self.status[p], self.markers[p] = EXITED, marker
            elif how == WALL:
                self.hits[p] += 1

    def read(self):
        return self.xy.copy(), self.cells.copy(), self.status.copy(), self.markers.copy(), self.hits.copy()


def random_particles(mesh, n, seed=0):
    """``n`` seeded positions strictly inside seeded cells of ``mesh``: (xy (n, 2), cells (n,))"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, mesh.num_cells, size=n)
    w = rng.uniform(0.05, 1.0, size=(n, 3))
    w /= w.sum(axis=1, keepdims=True)
    xy = (w[:, :, None]*mesh.cell_xy()[cells]).sum(axis=1)
    return xy, cells


def same_particles(got, want, label=''):
    """positions, cells, status, exit markers and wall hits: np.array_equal, each with a message that names the first difference"""
    for name, g, w in zip(('positions', 'cells', 'status', 'exit markers', 'wall hits'), got, want):
        if not np.array_equal(g, w):
            bad = np.nonzero(np.asarray(g != w).reshape(len(w), -1).any(axis=1))[0]
            raise AssertionError('{:} {:}: {:d} particles differ, first {:d}: {!r} != {!r}'.format(
                label, name, len(bad), int(bad[0]), g[bad[0]], w[bad[0]]))


# ---- closed forms
def midpoint_rotation(th):
    """one explicit-midpoint step of x' = w J x with th = w*dt is x -> ((1 - th^2/2) I + th J) x: (angle, radial factor)"""
    return math.atan2(th, 1.0 - 0.5*th*th), math.sqrt(1.0 + 0.25*th**4)


def rotated(xy0, centre, n_steps, th):
    """positions after ``n_steps`` midpoint steps of the solid-body rotation about ``centre``"""
    ang, fac = midpoint_rotation(th)
    a, r = n_steps*ang, fac**n_steps
    d = np.asarray(xy0, dtype=np.float64) - centre
    return centre + r*np.stack([np.cos(a)*d[:, 0] - np.sin(a)*d[:, 1], np.sin(a)*d[:, 0] + np.cos(a)*d[:, 1]], axis=1)


# ---- the scenarios both test files run: the CPU tests with the state frozen (and check there that the replay loses no particle
# ---- where none may be lost), the GPU tests with the state stepped between the moves
N_PARTICLES = 700               # three 256-lane workgroups, the last one partial


def scenario(name):
    """(mesh, bathymetry, uv, eta, time step, dt_move, open markers) of 'channel' (520 triangles, moves of about a quarter cell),
    'coast' (tests/golden/coast.msh: unstructured, concave boundary, marker ids 100 ...), 'long' (moves across five and more
    cells, many walls and exits) and 'cap' (1040 triangles, 80 along the channel: moves that reach the 64-cell cap)"""
    import os
    from helpers import channel_case
    if name == 'coast':
        from thetis_amd.meshio import read_gmsh
        mesh = read_gmsh(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh'))
        x, y = mesh.vertex_xy.T
        bath = 25.0 - 18.0*y/40e3 + 3.0*np.sin(x/9e3)
        rng = np.random.default_rng(5)
        uv = 0.2*rng.normal(size=(mesh.num_cells, 3, 2))
        eta = 0.2*rng.normal(size=(mesh.num_cells, 3))
        return mesh, bath, uv, eta, 0.2, 450.0, (100,)
    mesh, bath, uv, eta = channel_case(nx=40 if name == 'cap' else 20, ny=13, lx=100e3, ly=50e3, seed=21, amp_eta=0.3,
                                       amp_u=0.05 if name == 'cap' else 0.5)
    if name != 'channel':
        uv[:, :, 0] += 1.0                              # a drift along the channel on top of the noise
    return mesh, bath, uv, eta, 0.5, {'channel': 1200.0, 'long': 3.0e4, 'cap': 2.0e5}[name], (2,)
