"""
Section transports: the volume and tracer flux through lines across the domain - the discharge through a strait, the tidal prism
through an open boundary, the flux of a tracer or of suspended sediment through the same line - summed on the device
(csrc/swe2d_sections.hip) while ``FlowSolver2d.iterate`` keeps its batches.

    cb = SectionTransportCallback(solver_obj, sections={'strait': [(x0, y0), (x1, y1), (x2, y2)], 'inlet': 1},
                                  tracers=('salt_2d',), every=10)
    solver_obj.add_callback(cb, 'timestep')
    solver_obj.iterate()
    r = cb.result()          # r['time'], r['transport'][n_samples, n_sections], r['area'], r['tracer_transport'], r['cumulative_volume']

The reference has no 2D class for this (its ``TransectCallback`` is 3D only, thetis/callback.py:959).

The host resolves the geometry once.  ``cut_polyline`` cuts a polyline into PIECES - straight segments inside one cell - and hands
out, per piece, the cell, the barycentric weights of the cell's nodes at the piece's two Gauss-Legendre points and N = (nx, ny) len/2.
On a triangle u, eta, h and c are linear along a piece, H u.n c is a cubic and two points integrate it exactly, so the device needs no
geometry at all.  ``boundary_pieces`` gives one piece per exterior facet of a marker; along a cell edge every field is linear on
quadrilaterals too.  A piece contributes, without contraction and with f_q = fma(w_q[k-1], f[k-1], ... fma(w_q[1], f[1], w_q[0] f[0])),

    H_q = eta_q + h_q  (use_nonlinear_equations=False: h_q)      F_q = H_q fma(u_q, Nx, v_q Ny)      L = sqrt(Nx Nx + Ny Ny)
    transport  F_0 + F_1          area  L (H_0 + H_1)          tracer  fma(F_1, c_1, F_0 c_0)

and the terms of a section are added as limb sums (include/swe2d.h, swe2d_diagnostics_limbs): exact, whatever the order of the
pieces.  ``HostSections`` is the same arithmetic in numpy, bit for bit: the yardstick of the device and what the callback runs on a
device class without the section calls.
"""
import os
import warnings
import weakref
from fractions import Fraction

import numpy as np

from . import _lib
from .callback import DiagnosticCallback
from .pointeval import PointLocator, device_ready
from .timeintegrator import StepConsumer

__all__ = ['SectionTransportCallback', 'HostSections', 'Pieces', 'cut_polyline', 'boundary_pieces', 'section_pieces', 'fma',
           'split_limbs', 'limbs_to_double', 'LIMB_EXPONENTS']

LIMB_EXPONENTS = (40, 2, -36, -74, -112, -150)      # csrc/swe2d_kernels.h swe_sum_split: the units of the six limbs
_G = 1.0/np.sqrt(3.0)                               # the Gauss-Legendre points of [-1, 1] are -_G, +_G, both of weight 1
CUT_TOLERANCE = 1e-12                               # of cut_polyline, as a fraction of a polyline segment / in reference coordinates
# the other fixed numbers of cut_polyline; none of them decides which cell a piece belongs to (the midpoint rule does)
CUT_PARALLEL = 1e-14        # |d x e| <= this * |d| |e|: the edge is parallel to the segment and cuts nothing (rounding of one cross product)
CUT_EDGE_END = 1e-10        # a crossing counts while its position on the edge is in [-this, 1 + this]: a crossing at a vertex is never
                            # lost to rounding; a crossing counted in excess only splits a piece inside its cell in two
CUT_BOX_PAD = 1e-9          # edges are looked at when their box meets the segment's, both padded by this * the largest coordinate


# ---- exact arithmetic the device's terms are restated with
def _fma1(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a*b + c
    try:
        return float(Fraction(a)*Fraction(b) + Fraction(c))      # exact, rounded once (int/int division rounds to nearest even)
    except OverflowError:
        return a*b + c


_fma_ufunc = np.frompyfunc(_fma1, 3, 1)


def fma(a, b, c):
    """a*b + c rounded once, elementwise: what ``fma`` of the device computes (``math.fma`` is not in every Python)"""
    return np.asarray(_fma_ufunc(a, b, c), dtype=np.float64)


def split_limbs(x):
    """(limb sums [6] as Python integers, terms left out) of the terms ``x``: swe_sum_split / swe_sum_accumulate of
    csrc/swe2d_kernels.h.  A term that is not finite or not below 2^78 in magnitude is counted and not summed; every other term is
    split exactly into signed limbs of the units 2^40, 2^2, 2^-36, 2^-74, 2^-112, 2^-150 (what lies below is truncated)."""
    limbs, bad = [0]*len(LIMB_EXPONENTS), 0
    for v in np.asarray(x, dtype=np.float64).reshape(-1):
        v = float(v)
        if not abs(v) < 2.0**78:
            bad += 1
            continue
        r = Fraction(v)
        for j, s in enumerate(LIMB_EXPONENTS):
            unit = Fraction(2)**s
            t = int(r/unit)                      # truncation towards zero
            limbs[j] += t
            r -= t*unit
    return limbs, bad


def limbs_to_double(limbs):
    """the total of limb sums rounded to the nearest double, once (swe2d_sum_limbs_to_double)"""
    return float(sum(Fraction(int(v))*Fraction(2)**s for v, s in zip(limbs, LIMB_EXPONENTS)))


# ---- host geometry
class Pieces(object):
    """The pieces of one section: ``cell`` (n,), ``weights`` (n, 2, k) of the cell's nodes at the two Gauss points, ``normal``
    (n, 2) = (nx, ny)*len/2, ``length`` (n,), ``start`` / ``end`` (n, 2) the pieces' end points."""

    def __init__(self, cell, weights, normal, length, start, end):
        self.cell = np.ascontiguousarray(cell, dtype=np.int64)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.normal = np.ascontiguousarray(normal, dtype=np.float64)
        self.length = np.ascontiguousarray(length, dtype=np.float64)
        self.start = np.ascontiguousarray(start, dtype=np.float64)
        self.end = np.ascontiguousarray(end, dtype=np.float64)

    def __len__(self):
        return len(self.cell)

    @property
    def total_length(self):
        """the covered length of the section, metres"""
        return float(np.sum(self.length))


def _cross(a, b):
    return a[..., 0]*b[..., 1] - a[..., 1]*b[..., 0]


def cut_polyline(mesh, points, tolerance=CUT_TOLERANCE):
    """The pieces of the polyline through ``points`` [(x, y), ...] on the triangular ``mesh``: every segment of the polyline is cut
    where it meets a mesh edge, so a piece lies inside one cell and also ends at every polyline vertex.  Walked from the first point to
    the last, the normal of a piece is the RIGHT-HAND one, (dy, -dx)/len.

    Fixed rules: a piece belongs to the cell ``PointLocator`` gives for its midpoint (lowest-numbered cell whose closure holds it) -
    also a piece that runs along a mesh edge; parts of the polyline outside the mesh are dropped (``total_length`` is the covered
    length); cuts closer together than ``tolerance`` times the segment are one cut, so there is no piece of zero length; a polyline
    without any piece raises ``ValueError``.  The cuts of a segment are its intersections with ALL mesh edges whose box meets the
    segment's (no walk from neighbour to neighbour: O(edges) per segment, once), under the module's constants CUT_PARALLEL,
    CUT_EDGE_END and CUT_BOX_PAD, which are part of these rules.  Quadrilateral meshes: ``NotImplementedError`` (a bilinear field along a cut is not
    covered by the two-point rule)."""
    if int(mesh.cells.shape[1]) != 3:
        raise NotImplementedError('polyline sections on quadrilateral meshes are not supported: a bilinear field along a cut is '
                                  'not integrated exactly by the two-point rule (boundary-marker sections are)')
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(pts) < 2 or not np.isfinite(pts).all():
        raise ValueError('a polyline section needs at least two finite points')
    P = np.asarray(mesh.cell_xy(), dtype=np.float64)
    A = P.reshape(-1, 2)
    E = (np.roll(P, -1, axis=1) - P).reshape(-1, 2)
    e_len = np.hypot(E[:, 0], E[:, 1])
    lo, hi = np.minimum(A, A + E), np.maximum(A, A + E)
    pad = CUT_BOX_PAD*max(float(np.abs(P).max()), 1e-300)
    ta, tb, seg = [], [], []
    for j in range(len(pts) - 1):
        p, d = pts[j], pts[j + 1] - pts[j]
        L = float(np.hypot(d[0], d[1]))
        if L == 0.0:
            continue
        s_lo, s_hi = np.minimum(p, p + d) - pad, np.maximum(p, p + d) + pad
        near = np.nonzero(np.all((hi >= s_lo) & (lo <= s_hi), axis=1))[0]
        a, e = A[near], E[near]
        den = _cross(d, e)
        ok = np.abs(den) > CUT_PARALLEL*L*e_len[near]                  # (a parallel edge cuts nothing: its end points' other edges do)
        a, e, den = a[ok], e[ok], den[ok]
        t = _cross(a - p, e)/den                                # p + t d = a + s e
        s = _cross(a - p, d)/den
        t = t[(s >= -CUT_EDGE_END) & (s <= 1.0 + CUT_EDGE_END) & (t > 0.0) & (t < 1.0)]
        cuts = [0.0]
        for v in np.sort(t):
            if v - cuts[-1] > tolerance:
                cuts.append(float(v))
        if 1.0 - cuts[-1] > tolerance or len(cuts) == 1:
            cuts.append(1.0)
        else:
            cuts[-1] = 1.0
        ta.extend(cuts[:-1])
        tb.extend(cuts[1:])
        seg.extend([j]*(len(cuts) - 1))
    if not seg:
        raise ValueError('the polyline has no length')
    ta, tb, seg = np.array(ta), np.array(tb), np.array(seg)
    p0, d = pts[seg], pts[seg + 1] - pts[seg]
    tm, th = 0.5*(ta + tb), 0.5*(tb - ta)
    loc = PointLocator(mesh, p0 + tm[:, None]*d, tolerance=tolerance)
    keep = loc.cells >= 0
    if not keep.any():
        raise ValueError('the polyline lies outside the mesh: the section has no piece')
    ta, tb, tm, th, p0, d, cell = ta[keep], tb[keep], tm[keep], th[keep], p0[keep], d[keep], loc.cells[keep]
    w = np.stack([PointLocator._reference_coordinates(P[cell], p0 + (tm + sg*_G*th)[:, None]*d, tolerance)[1] for sg in (-1.0, 1.0)],
                 axis=1)
    normal = np.stack([d[:, 1], -d[:, 0]], axis=1)*th[:, None]
    length = (tb - ta)*np.hypot(d[:, 0], d[:, 1])
    return Pieces(cell, w, normal, length, p0 + ta[:, None]*d, p0 + tb[:, None]*d)


def boundary_pieces(mesh, marker):
    """One piece per exterior facet carrying boundary ``marker``, in the order of the cells: its end points are the facet's two
    vertices, its weights those of the facet's two nodes, its normal the OUTWARD one.  Triangles and quadrilaterals of either kind
    (along a cell edge every field is linear).  ``ValueError`` when no facet carries the marker."""
    nbr = np.asarray(mesh.cell_nbr)
    k = int(mesh.cells.shape[1])
    c, f = np.nonzero(nbr == -int(marker))
    if len(c) == 0:
        raise ValueError('no exterior facet carries boundary marker {:}: the section has no piece'.format(marker))
    P = np.asarray(mesh.cell_xy(), dtype=np.float64)
    g = (f + 1) % k
    a, b = P[c, f], P[c, g]
    d = b - a
    hi, lo = 0.5*(1.0 + _G), 0.5*(1.0 - _G)
    w = np.zeros((len(c), 2, k))
    idx = np.arange(len(c))
    w[idx, 0, f], w[idx, 0, g] = hi, lo
    w[idx, 1, f], w[idx, 1, g] = lo, hi
    normal = 0.5*np.stack([d[:, 1], -d[:, 0]], axis=1)             # counter-clockwise cells: the right-hand normal of a -> b is outward
    inward = np.sum(normal*(0.5*(a + b) - P[c].mean(axis=1)), axis=1) < 0.0
    normal[inward] = -normal[inward]
    return Pieces(c, w, normal, np.hypot(d[:, 0], d[:, 1]), a, b)


def section_pieces(mesh, spec):
    """``spec``: an int = a boundary marker (``boundary_pieces``), :class:`Pieces` cut earlier, else the points of a polyline
    (``cut_polyline``)"""
    if isinstance(spec, Pieces):
        return spec
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        return boundary_pieces(mesh, int(spec))
    return cut_polyline(mesh, spec)


# ---- the device's arithmetic in numpy
def _at(w, f):
    s = w[:, 0]*f[:, 0]
    for i in range(1, f.shape[1]):
        s = fma(w[:, i], f[:, i], s)
    return s


class HostSections(object):
    """The sums of csrc/swe2d_sections.hip in numpy.  ``sections``: one :class:`Pieces` (or None: an unused slot) per section slot."""

    def __init__(self, sections, use_nonlinear_equations=True):
        self.sections = list(sections)
        if len(self.sections) > _lib.MAX_SECTIONS:
            raise NotImplementedError('{:d} sections: at most SWE2D_MAX_SECTIONS = {:d} are supported'.format(
                len(self.sections), _lib.MAX_SECTIONS))
        self.nonlinear = bool(use_nonlinear_equations)

    def piece_terms(self, pieces, uv, eta, h, tracers=()):
        """(2 + n_tracers, n_pieces): transport, area and tracer terms of every piece, from the nodal values ``uv`` (N, k, 2),
        ``eta`` (N, k), the bathymetry at the cells' nodes ``h`` (N, k) and ``tracers`` [(N, k), ...]"""
        c = pieces.cell
        uv = np.asarray(uv, dtype=np.float64)
        u, v = uv[c, :, 0], uv[c, :, 1]
        e, hh = np.asarray(eta, dtype=np.float64)[c], np.asarray(h, dtype=np.float64)[c]
        w0, w1 = pieces.weights[:, 0, :], pieces.weights[:, 1, :]
        Nx, Ny = pieces.normal[:, 0], pieces.normal[:, 1]
        with np.errstate(all='ignore'):
            L = np.sqrt(Nx*Nx + Ny*Ny)
            h0, h1 = _at(w0, hh), _at(w1, hh)
            H0 = _at(w0, e) + h0 if self.nonlinear else h0
            H1 = _at(w1, e) + h1 if self.nonlinear else h1
            F0 = H0*fma(_at(w0, u), Nx, _at(w0, v)*Ny)
            F1 = H1*fma(_at(w1, u), Nx, _at(w1, v)*Ny)
            out = [F0 + F1, L*(H0 + H1)]
            for q in tracers:
                q = np.asarray(q, dtype=np.float64)[c]
                out.append(fma(F1, _at(w1, q), F0*_at(w0, q)))
        return np.stack(out)

    def eval_limbs(self, uv, eta, h, tracers=()):
        """(limb sums (MAX_SECTIONS, SECTION_VALUES, 6) int64, terms left out) - ``Swe2dDevice.sections_eval_limbs``"""
        if len(tracers) > _lib.MAX_SECTION_TRACERS:
            raise NotImplementedError('{:d} tracers: at most SWE2D_MAX_SECTION_TRACERS = {:d} are supported'.format(
                len(tracers), _lib.MAX_SECTION_TRACERS))
        limbs = np.zeros((_lib.MAX_SECTIONS, _lib.SECTION_VALUES, len(LIMB_EXPONENTS)), dtype=np.int64)
        bad = 0
        for s, pieces in enumerate(self.sections):
            if pieces is None or len(pieces) == 0:
                continue
            for q, terms in enumerate(self.piece_terms(pieces, uv, eta, h, tracers)):
                lq, nb = split_limbs(terms)
                limbs[s, q] = lq
                bad += nb
        return limbs, bad

    def eval(self, uv, eta, h, tracers=()):
        """(values (MAX_SECTIONS, SECTION_VALUES), terms left out) - ``Swe2dDevice.sections_eval``"""
        limbs, bad = self.eval_limbs(uv, eta, h, tracers)
        out = np.zeros(limbs.shape[:2])
        for s in range(limbs.shape[0]):
            for q in range(limbs.shape[1]):
                out[s, q] = limbs_to_double(limbs[s, q])
        return out, bad


# ---- the callback
class SectionTransportCallback(DiagnosticCallback, StepConsumer):
    """Volume and tracer transport through sections (see the module text).

    ``sections``: {name: polyline [(x, y), ...] | int boundary marker}.  NORMAL: for a polyline walked from its first to its last
    point the transport is counted along the right-hand normal (dy, -dx)/len - flow crossing the line from left to right is
    positive; for a boundary section along the outward normal - outflow is positive.  ``tracers``: labels of
    ``options.add_tracer_2d`` / 'sediment_2d' whose flux int H u.n c ds is summed as well (c: the tracer's solution field).
    DEPTH: H is the depth of the continuity term, eta + h with the device's current bathymetry (a bed moved by Exner counts), h
    alone with ``use_nonlinear_equations=False``.

    Per sample and section: ``transport`` int H u.n ds (m3/s), ``area`` int H ds (m2; transport/area is the section-mean normal
    velocity), per tracer ``tracer_transport``; ``length`` (m) is a constant of the section.  Register with
    ``add_callback(cb, 'timestep')`` - a sample after every ``every``-th step inside [start_time, end_time];
    ``FlowSolver2d.iterate`` keeps its batches, a sample is one small launch, the rows are read after the batch - or with 'export'.
    ``result()`` gives the arrays, ``history`` the samples as (time, transport, area, tracer_transport); unless
    ``export_to_hdf5=False`` rank 0 rewrites ``<output_directory>/diagnostic_<name>.npz`` at every export (there is no HDF5 sink).

    LIFETIME: the solver, this callback and the device refer to one another, so the device handle is freed by Python's cycle collector,
    not when the last name goes.  Freeing a handle synchronises and frees device memory: inside a stream capture of the same thread
    that invalidates the capture.  A script that captures graphs after dropping a solver should close its device first
    (``solver_obj.timestepper.device.close()``) or call ``gc.collect()`` before the capture.

    ``NotImplementedError``: polylines on quadrilateral meshes, wetting-drying, more than SWE2D_MAX_SECTIONS sections or
    SWE2D_MAX_SECTION_TRACERS tracers; several ranks at the first evaluation.  A section without any piece: ``ValueError``."""

    variable_names = ['transport', 'area', 'tracer_transport']

    def __init__(self, solver_obj, sections, tracers=(), every=1, name='sections', outputdir=None, append_to_log=True,
                 export_to_hdf5=True, start_time=None, end_time=None):
        self._history = []
        super(SectionTransportCallback, self).__init__(solver_obj, append_to_log=append_to_log, start_time=start_time,
                                                       end_time=end_time)
        self.name = name
        self.outputdir = outputdir
        self.export_to_hdf5 = export_to_hdf5
        self.every = int(every)
        if self.every < 1:
            raise ValueError('every must be >= 1')
        self.section_names = list(sections.keys())
        self.tracer_names = list(tracers)
        if len(self.section_names) > _lib.MAX_SECTIONS:
            raise NotImplementedError('{:d} sections: at most SWE2D_MAX_SECTIONS = {:d} are supported'.format(
                len(self.section_names), _lib.MAX_SECTIONS))
        if len(self.tracer_names) > _lib.MAX_SECTION_TRACERS:
            raise NotImplementedError('{:d} tracers: at most SWE2D_MAX_SECTION_TRACERS = {:d} are supported'.format(
                len(self.tracer_names), _lib.MAX_SECTION_TRACERS))
        self._refuse_wetting_and_drying()
        mesh = solver_obj.mesh2d
        self.pieces = [section_pieces(mesh, sections[n]) for n in self.section_names]
        self.length = np.array([p.total_length for p in self.pieces])
        self._host = HostSections(self.pieces, getattr(solver_obj.options, 'use_nonlinear_equations', True))
        self._dev = None
        self._pending = []                      # times of the rows appended on the device and not read yet
        self._time, self._rows, self._bad = [], [], []
        self._batch_iteration = 0
        self._warned = False

    # (DiagnosticCallback keeps a plain list; here rows of a batch may still be on the device)
    @property
    def history(self):
        self._flush()
        return self._history

    @history.setter
    def history(self, value):
        self._history = value

    def _refuse_wetting_and_drying(self):
        if getattr(self.solver_obj.options, 'use_wetting_and_drying', False):
            raise NotImplementedError('SectionTransportCallback with wetting-drying: the displaced depth of a partly dry piece is not '
                                      'covered by the two-point rule')

    # ---- where the sums are taken
    def _steppers(self):
        ts = self.solver_obj.timestepper
        out = [getattr(ts, 'swe', ts)]
        for label in self.tracer_names:
            d = getattr(self.solver_obj.fields[label], '_device_field', None)
            if d is not None:
                out.append(d[0])
        return out

    def _device(self):
        """the device with this callback's sections on it, or None on a device class without the section calls"""
        if getattr(self.solver_obj.comm, 'size', 1) > 1:
            raise NotImplementedError('SectionTransportCallback on several ranks: the partitioned driver does not carry sections yet '
                                      '(run the sections on one device)')
        self._refuse_wetting_and_drying()
        for label in self.tracer_names:
            if label not in self.solver_obj.fields:
                raise ValueError('SectionTransportCallback: the solver has no tracer {!r}'.format(label))
        dev = getattr(self._steppers()[0], 'device', None)
        if dev is None or not hasattr(dev, 'sections_set'):
            return None
        if self._dev is not None and self._dev is not dev:
            raise RuntimeError('the time stepper changed its device under a SectionTransportCallback')
        if self._dev is None:
            owner = getattr(dev, '_sections_owner', lambda: None)()      # (a weak reference: the device must not keep its callback alive)
            if owner is not None and owner is not self:
                raise RuntimeError('a device carries the sections of one SectionTransportCallback: give all sections to one callback')
            tids = [self.solver_obj.fields[label]._device_field[1] for label in self.tracer_names]
            n = [len(p) for p in self.pieces]
            dev.sections_set(len(self.pieces), np.repeat(np.arange(len(n)), n), np.concatenate([p.cell for p in self.pieces]),
                             np.concatenate([p.weights for p in self.pieces]), np.concatenate([p.normal for p in self.pieces]), tids)
            dev._sections_owner = weakref.ref(self)
            self._dev = dev
        return dev

    def _ready(self):
        return all(device_ready(s) for s in self._steppers())

    def _due(self, iteration, t):
        return iteration % self.every == 0 and self.start_time <= t <= self.end_time

    def _host_values(self):
        f = self.solver_obj.fields
        if hasattr(self.solver_obj, '_pull_bathymetry'):
            self.solver_obj._pull_bathymetry()
        return self._host.eval(f.uv_2d.cell_node_values(), f.elev_2d.cell_node_values(), f.bathymetry_2d.cell_node_values(),
                               [f[label].cell_node_values() for label in self.tracer_names])

    def _values_now(self):
        """((MAX_SECTIONS, SECTION_VALUES) of the state now, terms left out)"""
        dev = self._device()
        if dev is None:
            return self._host_values()
        if not self._ready():
            raise RuntimeError('SectionTransportCallback evaluated between the stages of a step')
        self._flush()
        return dev.sections_eval()

    def _split(self, row):
        ns, nt = len(self.section_names), len(self.tracer_names)
        return row[:ns, 0].copy(), row[:ns, 1].copy(), row[:ns, 2:2 + nt].copy()

    def _record(self, t, row, bad):
        self._time.append(float(t))
        self._rows.append(np.array(row))
        self._bad.append(int(bad))
        values = self._split(row)
        self._history.append((float(t),) + values)
        if bad and not self._warned:
            self._warned = True
            warnings.warn('{:}: {:d} terms of the sample at t = {:g} are not finite and were left out of the sums'.format(self.name, bad, t))
        if self.append_to_log:
            self.push_to_log(t, values)

    def _flush(self):
        """reads the rows a batch left on the device"""
        if self._pending:
            rows, bad = self._dev.sections_rows_read()
            pending, self._pending = self._pending, []
            if len(rows) != len(pending):
                raise RuntimeError('the device holds {:d} section rows, {:d} were appended'.format(len(rows), len(pending)))
            for t, r, b in zip(pending, rows, bad):
                self._record(t, r, b)

    # ---- samples of a batch (FlowSolver2d.create_iterator; the stepper's advance_steps asks per step of the batch)
    def row_probe(self, n_rows):
        if getattr(self.solver_obj.comm, 'size', 1) > 1:
            return None
        dev = self._device()
        if dev is None or not self._ready():
            return None
        self._flush()
        it = self.solver_obj.iteration
        need = (it + int(n_rows))//self.every - it//self.every          # multiples of `every` in (it, it + n_rows]
        if need > dev.sections_rows_capacity():
            dev.sections_rows_reserve(need)
        self._batch_iteration = it
        return dev, self

    def wants_append(self, k, t):
        """does step ``k`` of the batch, which ends at time ``t``, leave a sample?"""
        return self._due(self._batch_iteration + k + 1, t)

    def append(self, device, k, t):
        device.sections_rows_append()
        self._pending.append(t)

    # ---- one evaluation at a time
    def __call__(self):
        row, _ = self._values_now()
        return self._split(row)

    def evaluate(self, index=None):
        """a sample of the state now.  From the time loop's 'timestep' hook (``index`` None) on every ``every``-th step; at an
        export (``index``: the export's number) always."""
        t = self.solver_obj.simulation_time
        if index is None and not self._due(self.solver_obj.iteration, t):
            return
        if t < self.start_time or t > self.end_time:
            return
        self._flush()
        row, bad = self._values_now()
        self._record(t, row, bad)

    def message_str(self, transport, area, tracer_transport=None):
        return '{:}: '.format(self.name) + ', '.join('{:} Q = {:.6e} m3/s (A = {:.6e} m2)'.format(n, q, a)
                                                     for n, q, a in zip(self.section_names, transport, area))

    # ---- results
    def result(self):
        """dict: ``time`` (n,), ``transport`` (n, n_sections) m3/s, ``area`` (n, n_sections) m2, ``tracer_transport``
        (n, n_sections, n_tracers), ``cumulative_volume`` (n, n_sections) m3 - the trapezoid rule over the samples, 0 at the first -,
        ``length`` (n_sections,) m, ``n_unsummable`` (n,) terms left out of a sample because they were not finite"""
        self._flush()
        ns, nt, n = len(self.section_names), len(self.tracer_names), len(self._time)
        rows = np.array(self._rows, dtype=np.float64).reshape(n, _lib.MAX_SECTIONS, _lib.SECTION_VALUES)
        t = np.array(self._time, dtype=np.float64)
        q = rows[:, :ns, 0]
        cum = np.zeros((n, ns))
        for i in range(1, n):
            cum[i] = cum[i - 1] + 0.5*(q[i] + q[i - 1])*(t[i] - t[i - 1])
        return {'time': t, 'transport': q.copy(), 'area': rows[:, :ns, 1].copy(), 'tracer_transport': rows[:, :ns, 2:2 + nt].copy(),
                'cumulative_volume': cum, 'length': self.length.copy(), 'n_unsummable': np.array(self._bad, dtype=np.int64)}

    def export(self):
        """rank 0 rewrites diagnostic_<name>.npz with the samples so far (reads the rows of the last batch: one synchronisation)"""
        self._flush()
        if not self.export_to_hdf5 or getattr(self.solver_obj.comm, 'rank', 0) != 0:
            return
        data = self.result()
        data['section_names'] = np.array(self.section_names)
        data['tracer_names'] = np.array(self.tracer_names)
        outdir = self.outputdir or self.solver_obj.options.output_directory
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, 'diagnostic_{:}.npz'.format(self.name))
        tmp = path + '.tmp.npz'
        np.savez(tmp, **data)
        os.replace(tmp, path)
