"""
Harmonic tidal boundary forcing (the role of ``thetis/forcing.py``: ``TidalBoundaryForcing.set_tidal_field`` :1052):

    eta_b(x, t) = mean(x) + sum_k A_k(x) cos(omega_k t - phi_k(x))

``HarmonicTidalForcing`` holds the constituents as nodal tables on the space of an elevation field.  Used the reference's way - the
field as the boundary value, ``set_tidal_field`` called from ``update_forcings`` - it is a host function like any other forcing.
Given ITSELF as the boundary value,

    solver_obj.bnd_functions['shallow_water'] = {marker: {'elev': forcing}}

the time stepper evaluates the sum on the device in front of every Runge-Kutta stage (csrc/swe2d_tide.hip) and
``FlowSolver2d.iterate`` keeps its batches.  Both ways form ``omega_k*t - phi`` and the running sum left to right, in the order of
the constituents: they differ by the cosine routine only.
"""
import numpy as np

from . import _lib
from .function import Function
from .options import Constant

__all__ = ['HarmonicTidalForcing']


class HarmonicTidalForcing(object):
    def __init__(self, elev_field, omegas, amplitudes, phases, mean=None, boundary_ids=None):
        """
        :arg elev_field: scalar CG-P1 or DG-P1 :class:`Function` that :meth:`set_tidal_field` writes
        :arg omegas: (K,) angular frequencies [rad/s]
        :arg amplitudes, phases: (K, n_nodes) arrays, or lists of K Functions on ``elev_field``'s space (phases in rad)
        :kwarg mean: scalar, (n_nodes,) array or Function: the mean level (default 0)
        :kwarg boundary_ids: markers whose nodes :meth:`set_tidal_field` writes; None: every node (on the device path: every
            marker whose 'elev' is this object)
        The tables are copied: later changes of the arrays handed in are not seen.
        """
        if not isinstance(elev_field, Function):
            raise ValueError('elev_field must be a Function')
        fs = elev_field.function_space()
        if fs.vector or fs.degree != 1:
            raise ValueError('elev_field must be a scalar CG-P1 or DG-P1 Function')
        self.elev_field = elev_field
        n = fs.node_count()
        self.omegas = np.array(omegas, dtype=np.float64).reshape(-1)
        K = len(self.omegas)
        if K < 1:
            raise ValueError('at least one constituent is required')
        if K > _lib.MAX_TIDE_CONSTITUENTS:
            raise NotImplementedError('{:d} tidal constituents: at most SWE2D_MAX_TIDE_CONSTITUENTS = {:d} are supported'.format(
                K, _lib.MAX_TIDE_CONSTITUENTS))
        self.amplitudes = self._table(amplitudes, K, n, 'amplitudes')
        self.phases = self._table(phases, K, n, 'phases')
        if mean is None:
            self.mean = np.zeros(n)
        elif isinstance(mean, Function):
            self.mean = self._nodal(mean, n, 'mean')
        else:
            m = np.asarray(mean.values()[0] if isinstance(mean, Constant) else mean, dtype=np.float64)
            if m.ndim > 0 and m.shape != (n,):
                raise ValueError('mean must be a scalar or have one value per node of elev_field ({:d}), got shape {:}'.format(n, m.shape))
            self.mean = np.array(np.broadcast_to(m, (n,)), dtype=np.float64)
        if not (np.isfinite(self.omegas).all() and np.isfinite(self.amplitudes).all() and np.isfinite(self.phases).all()
                and np.isfinite(self.mean).all()):
            raise ValueError('the tidal tables must be finite')
        self.boundary_ids = None if boundary_ids is None else tuple(int(b) for b in np.atleast_1d(boundary_ids))
        self._nodes = None if self.boundary_ids is None else self._boundary_nodes(self.boundary_ids)

    def _nodal(self, f, n, what):
        fs, mine = f.function_space(), self.elev_field.function_space()
        if fs.mesh() is not mine.mesh() or fs.family != mine.family or fs.degree != mine.degree or fs.vector:
            raise ValueError('{:} must live on the function space of elev_field'.format(what))
        return np.array(f.dat.data_ro, dtype=np.float64).reshape(n)

    def _table(self, value, K, n, what):
        if isinstance(value, (list, tuple)) and len(value) > 0 and all(isinstance(v, Function) for v in value):
            if len(value) != K:
                raise ValueError('{:}: {:d} Functions for {:d} constituents'.format(what, len(value), K))
            return np.stack([self._nodal(v, n, what) for v in value])
        a = np.array(value, dtype=np.float64)
        if a.shape != (K, n):
            raise ValueError('{:} must have shape (K, n_nodes) = ({:d}, {:d}), got {:}'.format(what, K, n, a.shape))
        return a

    def _boundary_nodes(self, markers):
        """nodes of elev_field's space on the boundary facets that carry one of ``markers``"""
        fs = self.elev_field.function_space()
        mesh = fs.mesh()
        nbr = np.asarray(mesh.cell_nbr)
        cells = np.asarray(mesh.cells)
        npc = cells.shape[1]
        known = set(int(m) for m in mesh.boundary_markers)
        out = []
        for m in markers:
            if m not in known:
                raise ValueError('the mesh has no boundary with marker {:}'.format(m))
            c, f = np.nonzero(nbr == -m)
            for j in (f, (f + 1) % npc):
                out.append(cells[c, j] if fs.family == 'CG' else npc*c + j)
        return np.unique(np.concatenate(out))

    def evaluate(self, t, nodes=None):
        """the sum at time ``t`` at ``nodes`` (default: all) - THE expression, shared by every host path"""
        sl = slice(None) if nodes is None else nodes
        t = float(t)
        s = self.mean[sl].copy()
        for k in range(len(self.omegas)):
            s = s + self.amplitudes[k][sl]*np.cos(float(self.omegas[k])*t - self.phases[k][sl])
        return s

    def set_tidal_field(self, t):
        """writes the elevation of time ``t`` into ``elev_field`` (the nodes of ``boundary_ids``, or all)"""
        d = self.elev_field.dat.data                   # (a writable view: the field's host version moves on)
        if self._nodes is None:
            d[...] = self.evaluate(t)
        else:
            d[self._nodes] = self.evaluate(t, self._nodes)

    def facet_tables(self, device, marker):
        """(mean (n, 2), amp (K, n, 2), phase (K, n, 2)) at the end nodes of the boundary facets of ``marker``, in the order of
        ``device.boundary_facets``: what ``Swe2dDevice.tide_set`` takes"""
        fs = self.elev_field.function_space()
        mesh = fs.mesh()
        cov = mesh.cells if fs.family == 'CG' else None     # the same nodal injection CG -> DG as a Function-valued boundary

        def pick(a):
            if cov is None:
                a = a.reshape(mesh.num_cells, fs.npc)
            return device.facet_node_values(marker, a, cells_of_vertices=cov).values
        return (pick(self.mean), np.stack([pick(a) for a in self.amplitudes]), np.stack([pick(p) for p in self.phases]))
