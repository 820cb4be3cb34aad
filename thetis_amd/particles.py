"""
Lagrangian particle tracking: drifters advected in the depth-averaged velocity, on the device (csrc/swe2d_particles.hip).

    cb = ParticleTrackerCallback(solver_obj, [(x0, y0), (x1, y1), ...], every=10, open_boundaries=(1,))
    solver_obj.add_callback(cb, eval_interval='timestep')
    solver_obj.iterate()
    t, xy = cb.trajectories()          # (n_rows,), (n_rows, N, 2)
    cb.status()                        # ACTIVE / EXITED / LOST per particle

The reference has no 2D particle tracker.

After every ``every``-th step an ACTIVE particle makes one explicit-midpoint move of ``dt_move = every*dt`` in the velocity the step
left behind, frozen over the move.  Evaluated left to right, with + - * / and comparisons only:

    u1 = U(x, k);   (xm, km) = probe(x, k, (0.5*dt_move)*u1);   u2 = U(xm, km);   (x', k') = move(x, k, dt_move*u2)

``U(x, k)``: with the vertices p0, p1, p2 of cell k:  a = p1 - p0, b = p2 - p0, det = a.x*b.y - b.x*a.y, d = x - p0,
l1 = (d.x*b.y - b.x*d.y)/det, l2 = (a.x*d.y - d.x*a.y)/det, l0 = (1 - l1) - l2, and U = (l0*u0 + l1*u1) + l2*u2 of the cell's nodal
velocities.  The coordinate that vanishes on facet f (which joins the local vertices f, f + 1) is m_f = l_((f + 2) % 3).

``move(x, k, d)``: the straight walk along x -> y = x + d.  In the current cell form m_f(x) and m_f(y).  The candidates are the facets
with m_f(y) < 0, the facet just entered through excepted; without a candidate the particle arrives at (y, cell).  Else the candidate
with the smallest s_f = m_f(x)/(m_f(x) - m_f(y)) is crossed (ties: the lowest f).  An interior facet continues in the neighbour.  A
boundary facet whose marker is open sets EXITED, keeps the marker and freezes the particle at x + s*d.  Any other boundary is a
wall: the particle arrives at x + (s*(1 - 2^-10))*d in that cell, stays ACTIVE and counts a wall hit; it can leave the wall at the
next move.  A walk that has not arrived within MAX_HOPS = 64 cells makes the particle LOST at the position it had before the move:
a bound on the loop, not a tolerance.  ``probe`` is the same walk without consequences: an open boundary or a wall only ends it, at
the crossing or the shortened point; a probe that does not arrive makes the particle LOST as well.  EXITED and LOST particles are
never touched again.

Three things are opt-in per callback (``diffusivity=K, seed=s``, ``release_times=``, ``cell_counts()`` / ``concentration()``); a callback
without them runs what it ran before.

Random-walk dispersion (Visser 1997, uniform deviates) follows a midpoint move that arrived or ended at a wall, in the same launch.
With (x', k') where that move ended, dt = dt_move, K0, K1, K2 the diffusivity at the vertices of k' and l0, l1, l2 the coordinates of
x' as above, left to right:

    Kx = (l0*K0 + l1*K1) + l2*K2
    gx = ((K1-K0)*b.y - (K2-K0)*a.y)/det;   gy = (a.x*(K2-K0) - b.x*(K1-K0))/det          (constant per cell)
    Ko = Kx + (0.5*dt)*(gx*gx + gy*gy), a negative Ko is 0                                  (K half a drift step ahead, by the cell's own extension)
    amp = sqrt((6.0*dt)*Ko)                                                                 (sqrt(2 K dt/r), r = 1/3 the variance of R; np.sqrt)
    d = (dt*gx + amp*Rx, dt*gy + amp*Ry);   (x'', k'') = move(x', k', d)                     (d = (0, 0) is no walk)

``move`` is the walk above: an open boundary lets the particle exit, a wall stops it at the shortened point and counts one more hit (so
a move can count two; particles are not reflected), MAX_HOPS cells make it LOST at the position it had before the whole advance.
(w0, w1, w2, w3) = Philox4x32-10 of the counter (particle index, moves the set made before, 0, 0) under the key (seed & 0xffffffff,
seed >> 32), and Rx = 2*(((w0 >> 5)*67108864.0 + (w1 >> 6))*2^-53) - 1, Ry the same of w2, w3: in [-1, 1), every operation exact.  A
particle's deviates depend on (seed, index, move) alone - not on batching, the launch shape or the other particles.

Timed releases: a particle whose release time lies after the time at which the callback was made is WAITING (3) at its release
position.  It turns ACTIVE in the first move whose start time t - dt_move is >= its release time, and that move moves it already.

:class:`HostParticles` below is this algorithm in numpy - the documented restatement of the kernel, and the fallback of a device
class without particle sets.
"""
import os

import numpy as np

from . import _lib
from .callback import DiagnosticCallback
from .pointeval import PointLocator
from .timeintegrator import StepConsumer

__all__ = ['ParticleTrackerCallback', 'HostParticles', 'ACTIVE', 'EXITED', 'LOST', 'WAITING', 'MAX_HOPS', 'philox4x32_10', 'deviates']

ACTIVE, EXITED, LOST, WAITING = _lib.PARTICLE_ACTIVE, _lib.PARTICLE_EXITED, _lib.PARTICLE_LOST, _lib.PARTICLE_WAITING
MAX_HOPS = _lib.PARTICLE_MAX_HOPS
WALL_FACTOR = 1.0 - 2.0**-10
_ARRIVED, _EXIT, _WALL, _WALKING = 0, 1, 2, 3       # how a walk ended (_WALKING after MAX_HOPS cells: lost)
ROW_BUFFER_BYTES = 64 << 20                         # the default row buffer on the device: as many rows as fit, at least one


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011): ``counter`` (..., 4) and ``key`` (..., 2) 32-bit words -> (..., 4) uint32"""
    u64, mask = np.uint64, np.uint64(0xffffffff)
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = u64(0xD2511F53)*c0, u64(0xCD9E8D57)*c2             # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> u64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + u64(0x9E3779B9)) & mask, (k1 + u64(0xBB67AE85)) & mask
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def deviates(seed, index, move):
    """(Rx, Ry) in [-1, 1) of the particles ``index`` in move number ``move`` under the 64-bit ``seed`` (the module text)"""
    index = np.asarray(index, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    counter = np.stack([index, np.full_like(index, int(move) & 0xffffffff), np.zeros_like(index), np.zeros_like(index)], axis=-1)
    w = philox4x32_10(counter, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64)).astype(np.uint64)

    def one(a, b):
        return 2.0*(((a >> np.uint64(5)).astype(np.float64)*67108864.0 + (b >> np.uint64(6)).astype(np.float64))*2.0**-53) - 1.0
    return one(w[..., 0], w[..., 1]), one(w[..., 2], w[..., 3])


def vertex_diffusivity(value, n_vertices):
    """the (n_vertices,) table of a diffusivity given as a number or one value per vertex; ValueError unless finite and >= 0"""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n_vertices, float(a))
    if a.shape != (n_vertices,):
        raise ValueError('diffusivity: one value per vertex ({:d}), got shape {:}'.format(n_vertices, a.shape))
    if not (np.isfinite(a).all() and (a >= 0.0).all()):
        raise ValueError('diffusivity: the values must be finite and not negative')
    return np.array(a)


class HostParticles(object):
    """A particle set in numpy, by the formulas of csrc/swe2d_particles.hip (the module text), all particles at once.
    ``cells`` (N, 3), ``vertex_xy`` (V, 2), ``cell_nbr`` (N, 3) (a boundary facet: -marker), ``cell_nbr_facet`` (N, 3)."""

    def __init__(self, cells, vertex_xy, cell_nbr, cell_nbr_facet, xy, particle_cells):
        self.cv = np.asarray(cells, dtype=np.int64)
        self.vx, self.vy = (np.array(c, dtype=np.float64) for c in np.asarray(vertex_xy, dtype=np.float64).T)
        self.nbr = np.asarray(cell_nbr, dtype=np.int64)
        self.nbf = np.asarray(cell_nbr_facet, dtype=np.int64)
        self.xy = np.array(xy, dtype=np.float64).reshape(-1, 2)
        n = len(self.xy)
        self.cell = np.array(particle_cells, dtype=np.int64).reshape(n)
        self.status = np.full(n, ACTIVE, dtype=np.int32)
        self.marker = np.zeros(n, dtype=np.int32)
        self.hits = np.zeros(n, dtype=np.int32)
        self.rows = []
        self.kv, self.seed = None, 0                            # set_diffusivity: the vertex table and the key of the deviates
        self.release = None                                     # set_release_times
        self.n_moves = 0                                        # advance_at calls so far: the second counter word

    def set_diffusivity(self, diffusivity, seed=0):
        self.kv, self.seed = vertex_diffusivity(diffusivity, len(self.vx)), int(seed)

    def set_release_times(self, release_times, t_now=0.0):
        r = np.array(release_times, dtype=np.float64)
        if r.shape != self.status.shape or np.isnan(r).any():
            raise ValueError('release_times: one time per particle ({:d}), none of them NaN'.format(len(self.status)))
        self.release = r
        live = (self.status == ACTIVE) | (self.status == WAITING)
        self.status[live] = np.where(r[live] > float(t_now), WAITING, ACTIVE)

    def _geometry(self, k):
        v0, v1, v2 = self.cv[k, 0], self.cv[k, 1], self.cv[k, 2]
        x0, y0 = self.vx[v0], self.vy[v0]
        ax, ay = self.vx[v1] - x0, self.vy[v1] - y0
        bx, by = self.vx[v2] - x0, self.vy[v2] - y0
        return x0, y0, ax, ay, bx, by, ax*by - bx*ay

    @staticmethod
    def _facet_coordinates(g, px, py):
        """m_0, m_1, m_2 of the points in the cells of geometry ``g``"""
        x0, y0, ax, ay, bx, by, det = g
        dx, dy = px - x0, py - y0
        l1 = (dx*by - bx*dy)/det
        l2 = (ax*dy - dx*ay)/det
        l0 = (1.0 - l1) - l2
        return l2, l0, l1

    def _velocity(self, uv, k, px, py):
        m0, m1, m2 = self._facet_coordinates(self._geometry(k), px, py)
        w = uv[k]                                               # (n, 3, 2)
        return ((m1*w[:, 0, 0] + m2*w[:, 1, 0]) + m0*w[:, 2, 0], (m1*w[:, 0, 1] + m2*w[:, 1, 1]) + m0*w[:, 2, 1])

    def _walk(self, x, y, k, dx, dy, open_markers):
        """how, where (x, y, cell) and through which marker the walks along (x, y) -> (x + dx, y + dy) from the cells ``k`` end"""
        n = len(x)
        tx, ty = x + dx, y + dy
        how = np.full(n, _WALKING)
        ox, oy, ok, marker = x.copy(), y.copy(), k.copy(), np.zeros(n, dtype=np.int64)
        k, frm = k.copy(), np.full(n, -1)
        for _ in range(MAX_HOPS):
            w = np.nonzero(how == _WALKING)[0]
            if w.size == 0:
                break
            g = self._geometry(k[w])
            mx = self._facet_coordinates(g, x[w], y[w])
            my = self._facet_coordinates(g, tx[w], ty[w])
            best, sb = np.full(w.size, -1), np.zeros(w.size)
            for f in range(3):
                s = mx[f]/(mx[f] - my[f])
                take = (frm[w] != f) & (my[f] < 0.0) & ((best < 0) | (s < sb))
                best, sb = np.where(take, f, best), np.where(take, s, sb)
            here = best < 0
            a = w[here]
            how[a], ox[a], oy[a], ok[a] = _ARRIVED, tx[a], ty[a], k[a]
            w, best, sb = w[~here], best[~here], sb[~here]
            code = self.nbr[k[w], best]
            inner = code >= 0
            is_open = ~inner & np.isin(-code, open_markers)
            wall = ~inner & ~is_open
            e = w[is_open]
            how[e], ok[e], marker[e] = _EXIT, k[e], -code[is_open]
            ox[e], oy[e] = x[e] + sb[is_open]*dx[e], y[e] + sb[is_open]*dy[e]
            b = w[wall]
            f = sb[wall]*WALL_FACTOR
            how[b], ok[b], marker[b] = _WALL, k[b], -code[wall]
            ox[b], oy[b] = x[b] + f*dx[b], y[b] + f*dy[b]
            c = w[inner]
            frm[c] = self.nbf[k[c], best[inner]]
            k[c] = code[inner]
        return how, ox, oy, ok, marker

    def _dispersion(self, p, k, x, y, dt):
        """the random-walk displacement of the particles ``p`` at (x, y) in the cells ``k`` (the module text)"""
        g = self._geometry(k)
        _, _, ax, ay, bx, by, det = g
        m0, m1, m2 = self._facet_coordinates(g, x, y)
        K0, K1, K2 = self.kv[self.cv[k, 0]], self.kv[self.cv[k, 1]], self.kv[self.cv[k, 2]]
        Kx = (m1*K0 + m2*K1) + m0*K2
        gx = ((K1 - K0)*by - (K2 - K0)*ay)/det
        gy = (ax*(K2 - K0) - bx*(K1 - K0))/det
        Ko = Kx + (0.5*dt)*(gx*gx + gy*gy)
        Ko = np.where(Ko < 0.0, 0.0, Ko)
        amp = np.sqrt((6.0*dt)*Ko)
        rx, ry = deviates(self.seed, p, self.n_moves)
        return dt*gx + amp*rx, dt*gy + amp*ry

    def advance(self, uv, dt_move, open_markers=()):
        """one move of every ACTIVE particle in the nodal velocities ``uv`` (N, 3, 2)"""
        self._move(uv, dt_move, open_markers, False)

    def advance_at(self, uv, dt_move, t, open_markers=()):
        """``advance`` for a set with release times or a diffusivity: the move ends at time ``t`` and is counted"""
        dt_move = float(dt_move)
        if self.kv is not None and dt_move < 0.0:
            raise ValueError('a random walk cannot go back in time (dt_move < 0)')
        if self.release is not None:
            self.status[(self.status == WAITING) & (float(t) - dt_move >= self.release)] = ACTIVE
        self._move(uv, dt_move, open_markers, self.kv is not None)
        self.n_moves += 1

    def _move(self, uv, dt_move, open_markers, walk):
        uv = np.asarray(uv, dtype=np.float64).reshape(len(self.cv), 3, 2)
        open_markers = np.asarray(list(open_markers), dtype=np.int64)
        act = np.nonzero(self.status == ACTIVE)[0]
        if act.size == 0:
            return
        dt_move = float(dt_move)
        with np.errstate(all='ignore'):
            x, y, k = self.xy[act, 0].copy(), self.xy[act, 1].copy(), self.cell[act].copy()
            u, v = self._velocity(uv, k, x, y)
            half = 0.5*dt_move
            how, xm, ym, km, _ = self._walk(x, y, k, half*u, half*v, open_markers)
            lost = how == _WALKING
            km = np.where(lost, k, km)                          # (a lost probe has no midpoint: its second walk is discarded)
            u, v = self._velocity(uv, km, xm, ym)
            how, xn, yn, kn, marker = self._walk(x, y, k, dt_move*u, dt_move*v, open_markers)
            lost |= how == _WALKING
            hits = (how == _WALL).astype(np.int32)
            if walk:
                w = np.nonzero(~lost & ((how == _ARRIVED) | (how == _WALL)))[0]
                dx, dy = self._dispersion(act[w], kn[w], xn[w], yn[w], dt_move)
                go = (dx != 0.0) | (dy != 0.0)                  # (a zero displacement is no walk)
                w, dx, dy = w[go], dx[go], dy[go]
                how[w], xn[w], yn[w], kn[w], marker[w] = self._walk(xn[w], yn[w], kn[w], dx, dy, open_markers)
                lost |= how == _WALKING
                hits[w] += how[w] == _WALL
        self.status[act[lost]] = LOST
        ok = ~lost
        a = act[ok]
        self.xy[a, 0], self.xy[a, 1], self.cell[a] = xn[ok], yn[ok], kn[ok]
        ex = ok & (how == _EXIT)
        self.status[act[ex]] = EXITED
        self.marker[act[ex]] = marker[ex]
        self.hits[a] += hits[ok]

    def cell_counts(self, status=(ACTIVE,)):
        """(n_cells,) int32: the particles of the listed status in every cell"""
        sel = np.isin(self.status, np.asarray(list(status), dtype=np.int64))
        return np.bincount(self.cell[sel], minlength=len(self.cv)).astype(np.int32)

    def record(self):
        self.rows.append(self.xy.copy())

    def read(self):
        return self.xy.copy(), self.cell.astype(np.int32), self.status.copy(), self.marker.copy(), self.hits.copy()

    def read_rows(self):
        rows, self.rows = self.rows, []
        return np.array(rows, dtype=np.float64).reshape(len(rows), len(self.xy), 2)


class ParticleTrackerCallback(DiagnosticCallback, StepConsumer):
    """Particles released at ``positions`` (N, 2) and advected with the flow (see the module text).  Register with
    ``add_callback(cb, eval_interval='timestep')``: after a step whose iteration count is a multiple of ``every`` and whose time lies
    in [start_time, end_time] the particles move by ``dt_move = every*dt``; after every ``record_every``-th move the positions are
    kept as a row of ``trajectories()``.  Particles leave through the boundaries listed in ``open_boundaries`` (markers); every other
    boundary is a wall.  ``FlowSolver2d.iterate`` keeps its batches, and the steps between two moves go to the device in one call.

    A device class without particle sets (the host stand-in of the tests) runs :class:`HostParticles` from the fields' nodal values,
    step by step.  Several ranks: ``NotImplementedError`` at the first evaluation; a quadrilateral mesh: at construction; a position
    outside the mesh: ``PointNotInDomainError`` at construction.  Unless ``export_to_hdf5=False`` rank 0 rewrites
    ``<output_directory>/diagnostic_<name>.npz`` at every export.  ``row_capacity``: rows the device keeps before the callback
    reads them back (default: what fits 64 MiB).

    ``diffusivity=K`` (a non-negative number or ``Constant``, a CG-P1 ``Function`` or one value per vertex) adds the random-walk
    dispersion of the module text to every move, with the deviates of ``seed`` (a 64-bit integer); a DG or vector ``K``:
    ``NotImplementedError``.  ``release_times`` (N,), in simulation time: a particle whose time lies after the time at which the
    callback is made is WAITING at its release point until a move starts at or after its time.  ``cell_counts()`` and
    ``concentration()`` turn the cloud into a field.  A set with a diffusivity or release times goes through
    ``particles_advance_at``; a device class with particle sets but without that call runs :class:`HostParticles`."""

    def __init__(self, solver_obj, positions, name='particles', every=1, record_every=1, open_boundaries=(), start_time=None,
                 end_time=None, export_to_hdf5=True, outputdir=None, row_capacity=None, diffusivity=None, seed=0, release_times=None):
        super(ParticleTrackerCallback, self).__init__(solver_obj, append_to_log=False, start_time=start_time, end_time=end_time)
        self.name = name
        self.export_to_hdf5 = export_to_hdf5
        self.outputdir = outputdir
        self.every, self.record_every = int(every), int(record_every)
        if self.every < 1 or self.record_every < 1:
            raise ValueError('every and record_every must be >= 1')
        mesh = solver_obj.mesh2d
        if np.asarray(mesh.cells).shape[1] != 3:
            raise NotImplementedError('ParticleTrackerCallback: particles are tracked on triangles only')
        self.open_boundaries = tuple(int(m) for m in open_boundaries)
        self.initial_positions = np.array(positions, dtype=np.float64).reshape(-1, 2)
        loc = PointLocator(mesh, self.initial_positions, tolerance=0.5e-12)     # (swe2d_particles_create admits -1e-12)
        loc.check()
        self.initial_cells = loc.cells.copy()
        n = len(self.initial_positions)
        self.row_capacity = int(row_capacity) if row_capacity is not None else max(1, min(1024, ROW_BUFFER_BYTES//(16*max(n, 1))))
        if self.row_capacity < 1:
            raise ValueError('row_capacity must be >= 1')
        self.seed = int(seed)
        if not 0 <= self.seed < 2**64:
            raise ValueError('seed must be a 64-bit unsigned integer')
        self.diffusivity = None if diffusivity is None else self._vertex_table(diffusivity, mesh)
        self.release_times = None
        self._t_made = float(getattr(solver_obj, 'simulation_time', 0.0))
        if release_times is not None:
            self.release_times = np.array(release_times, dtype=np.float64)
            if self.release_times.shape != (n,) or np.isnan(self.release_times).any():
                raise ValueError('release_times: one time per particle, shape ({:d},), none of them NaN'.format(n))
        self._timed_or_walking = self.diffusivity is not None or self.release_times is not None
        self.n_advances = 0
        self._times = []                                # the times of the recorded rows
        self._rows = []                                 # rows already read back, (r, N, 2) blocks
        self._on_device = 0                             # rows in the device's buffer
        self._set = None                                # (device, particle set id)
        self._host = None                               # HostParticles of a device class without particle sets
        self._batch_iteration = 0

    @staticmethod
    def _vertex_table(K, mesh):
        """the per-vertex table of the diffusivity ``K``"""
        from .function import Function
        if isinstance(K, Function):
            fs = K.function_space()
            if fs.family != 'CG' or fs.degree != 1 or fs.vector:
                raise NotImplementedError('ParticleTrackerCallback: the diffusivity {!r} lives in a {:}{:d}{:} space; the random walk '
                                          'takes a constant or a scalar CG-P1 field'.format(K.name(), fs.family, fs.degree,
                                                                                            ' vector' if fs.vector else ''))
            K = K.dat.data_ro
        elif not isinstance(K, np.ndarray):
            K = float(K)                                # a number or a Constant
        return vertex_diffusivity(K, mesh.num_vertices)

    # ---- where the particles live
    def _stepper(self):
        stepper = self.solver_obj.timestepper
        return getattr(stepper, 'swe', stepper)

    def _device_set(self):
        """(device, particle set id) on a device class with particle sets, else None"""
        if getattr(self.solver_obj.comm, 'size', 1) > 1:
            raise NotImplementedError('ParticleTrackerCallback on several ranks: the partitioned driver does not carry particle '
                                      'sets (track the particles on one device)')
        dev = getattr(self._stepper(), 'device', None)
        if dev is None or not hasattr(dev, 'particles_create') or (self._timed_or_walking and not hasattr(dev, 'particles_advance_at')):
            return None
        if self._set is not None and self._set[0] is not dev:
            raise RuntimeError('the time stepper changed its device under a ParticleTrackerCallback')
        if self._set is None:
            self._set = (dev, dev.particles_create(self.initial_positions, self.initial_cells, capacity=self.row_capacity))
            if self.diffusivity is not None:
                dev.particles_set_diffusivity(self._set[1], self.diffusivity, self.seed)
            if self.release_times is not None:
                dev.particles_set_release_times(self._set[1], self.release_times, self._t_made)
        return self._set

    def _host_set(self):
        if self._host is None:
            mesh = self.solver_obj.mesh2d
            self._host = HostParticles(mesh.cells, mesh.vertex_xy, mesh.cell_nbr, mesh.cell_nbr_facet, self.initial_positions,
                                       self.initial_cells)
            if self.diffusivity is not None:
                self._host.set_diffusivity(self.diffusivity, self.seed)
            if self.release_times is not None:
                self._host.set_release_times(self.release_times, self._t_made)
        return self._host

    def _due(self, iteration, t):
        return iteration % self.every == 0 and self.start_time <= t <= self.end_time

    def _dt_move(self):
        return self.every*self.solver_obj.dt

    def _drain(self):
        if self._set is not None and self._on_device:
            self._rows.append(self._set[0].particles_read_rows(self._set[1]))
            self._on_device = 0
        elif self._host is not None and self._host.rows:
            self._rows.append(self._host.read_rows())

    def _sample(self, t, device=None, uv=None):
        """one move at time ``t`` (on ``device``, or on the host in the nodal velocities ``uv``) and, when due, one row"""
        if not self._timed_or_walking:                  # the set is advanced as it always was
            if device is not None:
                device.particles_advance(self._set[1], self._dt_move(), self.open_boundaries)
            else:
                self._host_set().advance(uv, self._dt_move(), self.open_boundaries)
        elif device is not None:
            device.particles_advance_at(self._set[1], self._dt_move(), t, self.open_boundaries)
        else:
            self._host_set().advance_at(uv, self._dt_move(), t, self.open_boundaries)
        self.n_advances += 1
        if self.n_advances % self.record_every:
            return
        if device is not None:
            if self._on_device >= self.row_capacity:
                self._drain()                           # before the buffer fills: one synchronisation per row_capacity rows
            device.particles_record(self._set[1])
            self._on_device += 1
        else:
            self._host.record()
        self._times.append(t)

    # ---- moves of a batch (FlowSolver2d.create_iterator; the stepper's advance_steps asks per step of the batch)
    def row_probe(self, n_rows):
        from .pointeval import device_ready
        if getattr(self.solver_obj.comm, 'size', 1) > 1 or not device_ready(self._stepper()):
            return None
        s = self._device_set()
        if s is None:
            return None
        self._batch_iteration = self.solver_obj.iteration
        return s[0], self

    def wants_append(self, k, t):
        """does step ``k`` of the batch, which ends at time ``t``, move the particles?"""
        return self._due(self._batch_iteration + k + 1, t)

    def append(self, device, k, t):
        self._sample(t, device=device)

    # ---- one step at a time
    def evaluate(self, index=None):
        t = self.solver_obj.simulation_time
        s = self._device_set()
        if not self._due(self.solver_obj.iteration, t):
            return
        if s is not None:
            from .pointeval import device_ready
            if not device_ready(self._stepper()):
                raise RuntimeError('ParticleTrackerCallback evaluated between the stages of a step')
            self._sample(t, device=s[0])
            return
        assert self._set is None, 'this callback tracks its particles on the device'
        self._sample(t, uv=self.solver_obj.fields.uv_2d.cell_node_values())

    # ---- results
    def _read(self):
        if self._set is not None:
            return self._set[0].particles_read(self._set[1])
        if self._host is not None:
            return self._host.read()
        n = len(self.initial_positions)
        status = np.full(n, ACTIVE, dtype=np.int32)
        if self.release_times is not None:
            status[self.release_times > self._t_made] = WAITING
        return (self.initial_positions.copy(), self.initial_cells.astype(np.int32), status, np.zeros(n, dtype=np.int32),
                np.zeros(n, dtype=np.int32))

    def positions(self):
        """(N, 2) current positions (an EXITED particle: where it crossed the boundary); synchronises"""
        return self._read()[0]

    def cells(self):
        return self._read()[1]

    def status(self):
        """(N,) ACTIVE / EXITED / LOST / WAITING"""
        return self._read()[2]

    def exit_markers(self):
        """(N,) the boundary marker an EXITED particle left through, 0 otherwise"""
        return self._read()[3]

    def wall_hits(self):
        """(N,) moves that ended at a wall"""
        return self._read()[4]

    def trajectories(self):
        """(times (n_rows,), positions (n_rows, N, 2)): the rows recorded so far; synchronises"""
        self._drain()
        n = len(self.initial_positions)
        rows = np.concatenate(self._rows) if self._rows else np.zeros((0, n, 2))
        self._rows = [rows]
        assert len(rows) == len(self._times), 'the set holds {:d} rows, the host counted {:d}'.format(len(rows), len(self._times))
        return np.array(self._times, dtype=np.float64), rows

    def cell_counts(self, status=(ACTIVE,)):
        """(n_cells,) int32 in the mesh's numbering: the particles of the listed status in every cell; synchronises"""
        status = tuple(int(s) for s in status)
        if self._set is not None:
            return self._set[0].particles_cell_counts(self._set[1], status)
        if self._host is not None:
            return self._host.cell_counts(status)
        _, cells, st, _, _ = self._read()
        return np.bincount(cells[np.isin(st, status)], minlength=self.solver_obj.mesh2d.num_cells).astype(np.int32)

    def concentration(self, status=(ACTIVE,)):
        """a DG0 ``Function``: particles per unit area in every cell"""
        from .function import Function, get_functionspace
        mesh = self.solver_obj.mesh2d
        return Function(get_functionspace(mesh, 'DG', 0), name='{:}_concentration'.format(self.name)).assign(
            self.cell_counts(status)/mesh.cell_areas())

    def excursion(self):
        """(N,) distance of every particle from its release point"""
        return np.hypot(*(self.positions() - self.initial_positions).T)

    def __call__(self):
        return (self.n_advances,)

    def message_str(self, *values):
        return '{:}: {:d} moves'.format(self.name, values[0])

    def export(self):
        """rank 0 rewrites diagnostic_<name>.npz: time (n_rows,), trajectories (n_rows, N, 2), positions, cells, status, exit_markers,
        wall_hits, initial_positions, and of a set with them release_times, seed, diffusivity (per vertex) - one read-back of the particle state and of the rows not read yet"""
        if not self.export_to_hdf5 or getattr(self.solver_obj.comm, 'rank', 0) != 0:
            return
        t, rows = self.trajectories()
        xy, cells, status, markers, hits = self._read()
        data = {'time': t, 'trajectories': rows, 'positions': xy, 'cells': cells, 'status': status, 'exit_markers': markers,
                'wall_hits': hits, 'initial_positions': self.initial_positions, 'n_advances': np.array(self.n_advances),
                'dt_move': np.array(self._dt_move()), 'open_boundaries': np.array(self.open_boundaries, dtype=np.int64)}
        if self._timed_or_walking:
            data['seed'] = np.array(self.seed, dtype=np.uint64)
            if self.release_times is not None:
                data['release_times'] = self.release_times
            if self.diffusivity is not None:
                data['diffusivity'] = self.diffusivity
        outdir = self.outputdir or self.solver_obj.options.output_directory
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, 'diagnostic_{:}.npz'.format(self.name))
        tmp = path + '.tmp.npz'
        np.savez(tmp, **data)
        os.replace(tmp, path)
