"""
Point location on the host: which cell holds a point, and the nodal weights that evaluate a P1 / Q1 field there.

``PointLocator(mesh, points)`` finds, for every point, its cell (the caller's numbering) and its weights - 3 barycentric weights on
triangles, 4 bilinear weights on quadrilaterals in the DQ-1 node order of ``function.quadrilateral_quadrature`` (the bilinear map is
inverted by Newton's method, parallelograms in closed form).  Candidate cells come from a bucket grid over the cells' bounding
boxes, so the cost is O(N_cells + N_points * cells per bucket), never N_cells x N_points.  The geometry is ``mesh.cell_xy()``:
periodic meshes, whose cells are stored unwrapped, need nothing special.

Tie rule: a point on a shared facet or vertex belongs to the lowest-numbered cell whose closure contains it within ``tolerance``
(reference coordinates): deterministic and independent of any partition.  A point inside the tolerance band but outside the cell
is extrapolated, not clamped.

The device gathers with these weights (csrc/swe2d_probe.hip); ``evaluate`` is the same sum on host arrays, left to right.
"""
import numpy as np

__all__ = ['PointLocator', 'PointNotInDomainError', 'select_and_move_detectors', 'evaluate']

DEFAULT_TOLERANCE = 1e-10


class PointNotInDomainError(Exception):
    """A point (detector) lies outside the mesh (firedrake.PointNotInDomainError's role)."""

    def __init__(self, point, name=None):
        self.point = tuple(float(v) for v in point)
        self.name = name
        what = 'detector {!r} at '.format(name) if name is not None else 'point '
        super(PointNotInDomainError, self).__init__('{:}({:g}, {:g}) is not in the domain'.format(what, *self.point))


def _cross(u, v):
    return u[..., 0]*v[..., 1] - u[..., 1]*v[..., 0]


class PointLocator(object):
    """``cells`` (M,) int64 (-1: outside the mesh) and ``weights`` (M, k) of ``points`` (M, 2) on ``mesh``."""

    def __init__(self, mesh, points, tolerance=None):
        tol = DEFAULT_TOLERANCE if tolerance is None else float(tolerance)
        pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        P = np.asarray(mesh.cell_xy(), dtype=np.float64)
        n, k = P.shape[0], P.shape[1]
        self.points, self.npc, self.tolerance = pts, k, tol
        m = pts.shape[0]
        self.cells = np.full(m, -1, dtype=np.int64)
        self.weights = np.zeros((m, k))
        if m == 0:
            return
        lo, hi = P.min(axis=1), P.max(axis=1)
        span = hi - lo
        pad = tol*span.max(axis=1, keepdims=True) + 1e-12*np.abs(P).max()
        lo, hi = lo - pad, hi + pad
        # bucket grid: about one cell per bucket
        g0, g1 = lo.min(axis=0), hi.max(axis=0)
        ext = np.maximum(g1 - g0, 1e-300)
        h = max(np.sqrt(ext[0]*ext[1]/max(n, 1)), 1e-300)
        nb = np.clip(np.ceil(ext/h).astype(np.int64), 1, 4096)

        def bucket(xy):
            return np.clip(((xy - g0)/ext*nb).astype(np.int64), 0, nb - 1)
        b0, b1 = bucket(lo), bucket(hi)
        cnt = (b1 - b0 + 1).prod(axis=1)
        cell_of = np.repeat(np.arange(n), cnt)
        # position of every (cell, bucket) pair inside its cell's box, row-major
        start = np.cumsum(cnt) - cnt
        r = np.arange(cell_of.size) - start[cell_of]
        w = (b1 - b0 + 1)[cell_of, 0]
        bx = b0[cell_of, 0] + r % w
        by = b0[cell_of, 1] + r//w
        key = by*nb[0] + bx
        order = np.argsort(key, kind='stable')                 # cells ascending inside every bucket
        key, cell_of = key[order], cell_of[order]
        off = np.searchsorted(key, np.arange(nb[0]*nb[1] + 1))
        # candidate (point, cell) pairs
        pb = bucket(pts)
        inside_grid = np.all((pts >= g0) & (pts <= g1), axis=1)
        pk = pb[:, 1]*nb[0] + pb[:, 0]
        pc = np.where(inside_grid, off[pk + 1] - off[pk], 0)
        pt_of = np.repeat(np.arange(m), pc)
        pstart = np.cumsum(pc) - pc
        cand = cell_of[off[pk[pt_of]] + np.arange(pt_of.size) - pstart[pt_of]]
        ok, wts = self._reference_coordinates(P[cand], pts[pt_of], tol)
        # lowest inside cell per point: candidates are ascending by cell inside a point's segment
        hit = np.nonzero(ok)[0]
        if hit.size:
            first = np.unique(pt_of[hit], return_index=True)
            sel = hit[first[1]]
            self.cells[pt_of[sel]] = cand[sel]
            self.weights[pt_of[sel]] = wts[sel]

    @staticmethod
    def _reference_coordinates(P, x, tol):
        """(inside within tol, weights) of points x (n, 2) in cells P (n, k, 2)"""
        if P.shape[1] == 3:
            a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
            d = x - P[:, 0]
            det = _cross(a, b)
            l1 = _cross(d, b)/det
            l2 = _cross(a, d)/det
            l0 = 1.0 - l1 - l2
            ok = (l0 >= -tol) & (l1 >= -tol) & (l2 >= -tol)
            return ok, np.stack([l0, l1, l2], axis=1)
        a, b = P[:, 1] - P[:, 0], P[:, 3] - P[:, 0]
        c = P[:, 0] - P[:, 1] + P[:, 2] - P[:, 3]
        d = x - P[:, 0]
        det = _cross(a, b)
        xi = _cross(d, b)/det                                   # parallelograms: exact (c = 0)
        ze = _cross(a, d)/det
        scale = np.abs(P).max()
        gen = np.abs(c).max(axis=1) > 1e-14*max(scale, 1e-300)
        if gen.any():
            # x(xi, ze) = p0 + xi a + ze b + xi ze c: Newton from the parallelogram guess
            ag, bg, cg, dg = a[gen], b[gen], c[gen], d[gen]
            u, v = xi[gen], ze[gen]
            for _ in range(30):
                rx = u[:, None]*ag + v[:, None]*bg + (u*v)[:, None]*cg - dg
                ju, jv = ag + v[:, None]*cg, bg + u[:, None]*cg
                jd = _cross(ju, jv)
                du = _cross(rx, jv)/jd
                dv = _cross(ju, rx)/jd
                u, v = u - du, v - dv
                if max(np.abs(du).max(), np.abs(dv).max()) < 1e-15:
                    break
            xi[gen], ze[gen] = u, v
            # Newton may stall on a candidate far from the point (a root of the bilinear map outside the cell): keep converged roots only
            rx = u[:, None]*ag + v[:, None]*bg + (u*v)[:, None]*cg - dg
            size = np.abs(ag).max(axis=1) + np.abs(bg).max(axis=1)
            conv = np.zeros(len(xi), dtype=bool)
            conv[gen] = np.abs(rx).max(axis=1) <= 1e-10*size
            xi[gen & ~conv] = np.nan
        ok = (xi >= -tol) & (xi <= 1.0 + tol) & (ze >= -tol) & (ze <= 1.0 + tol)
        return ok, np.stack([(1 - xi)*(1 - ze), xi*(1 - ze), xi*ze, (1 - xi)*ze], axis=1)

    def check(self, names=None):
        """raise PointNotInDomainError for the first point outside the mesh"""
        bad = np.nonzero(self.cells < 0)[0]
        if bad.size:
            i = int(bad[0])
            raise PointNotInDomainError(self.points[i], None if names is None else names[i])


def evaluate(cell_node_values, cells, weights):
    """The probe's sum on host arrays: ``cell_node_values`` (N, k[, c]) -> (M[, c]), w0*v0 + w1*v1 + ... left to right."""
    v = np.asarray(cell_node_values)[np.asarray(cells)]
    w = np.asarray(weights)
    if v.ndim == 3:
        w = w[:, :, None]
    s = w[:, 0]*v[:, 0]
    for i in range(1, v.shape[1]):
        s = s + w[:, i]*v[:, i]
    return s


def device_ready(stepper):
    """Sync a device stepper's host edits to the device; False when its buffer A does not hold what a host read would see (a
    reader between the stages of a step: the host copy then is the last completed stage)"""
    stepper._sync_to_device()
    return not (getattr(stepper, '_device_ahead', False) and getattr(stepper, '_last_stage', 2) != 2)


def probe_once(stepper, field, cells, weights, cache_size=8):
    """(M, components) of ``field`` ('uv', 'elev' or a tracer id) of ``stepper.device`` at located points, by a probe set kept in
    a small cache on the stepper; None when the device state cannot be read this way (see device_ready)"""
    from collections import OrderedDict
    if not device_ready(stepper):
        return None
    dev = stepper.device
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if len(cells) == 0:
        return np.zeros((0, 2 if field == 'uv' else 1))
    cache = stepper.__dict__.setdefault('_probe_cache', OrderedDict())
    key = (field, cells.tobytes(), weights.tobytes())
    pid = cache.get(key)
    if pid is None:
        pid = dev.probe_create(cells, weights, [field])
        cache[key] = pid
        if len(cache) > cache_size:
            dev.probe_destroy(cache.popitem(last=False)[1])
    else:
        cache.move_to_end(key)
    return dev.probe_eval(pid)


def select_and_move_detectors(mesh, detector_locations, detector_names=None, maximum_distance=0.):
    """Select the detectors inside the domain; a detector outside moves to the nearest cell centroid when that lies within
    ``maximum_distance`` and is dropped otherwise (thetis/utility.py:864-930).  Equal distances are broken lexicographically on
    the centroid coordinates.  Returns the accepted locations, and with ``detector_names`` also their names."""
    locs = [tuple(float(v) for v in loc) for loc in detector_locations]
    names = [None]*len(locs) if detector_names is None else list(detector_names)
    found = PointLocator(mesh, locs).cells if locs else np.zeros(0, dtype=np.int64)
    cen = None
    accepted, accepted_names = [], []
    for loc, name, cell in zip(locs, names, found):
        if cell < 0:
            if cen is None:
                cen = np.asarray(mesh.cell_xy(), dtype=np.float64).mean(axis=1)
            dist = np.sqrt((cen[:, 0] - loc[0])**2 + (cen[:, 1] - loc[1])**2)
            i = np.lexsort((cen[:, 1], cen[:, 0], dist))[0]
            if dist[i] > maximum_distance:
                continue
            loc = (float(cen[i, 0]), float(cen[i, 1]))
        accepted.append(list(loc))
        accepted_names.append(name)
    if detector_names is None:
        return accepted
    return accepted, accepted_names
