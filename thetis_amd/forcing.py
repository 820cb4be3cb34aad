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

Atmospheric forcing (``thetis/forcing.py``: ``compute_wind_stress`` :19, ``AtmosphericForcingInterpolator.set_fields`` :148): a record
of 10 m wind and mean-sea-level pressure snapshots, interpolated linearly in time, the wind turned into wind stress.
``AtmosphericForcing`` holds the snapshots as per-vertex tables.  Used the reference's way - the two fields as option values,
``set_fields`` called from ``update_forcings`` - it is a host function.  Given ITSELF as the option value,

    options.wind_stress = forcing;  options.atmospheric_pressure = forcing

the device holds the record and evaluates both fields in front of every Runge-Kutta stage (csrc/swe2d_atm.hip); ``iterate`` keeps its
batches.  Both ways form the same expressions in the same order: they differ by the rounding of the square root at most.
"""
import numpy as np

from . import _lib
from .function import Function
from .options import Constant
from .shallowwater_eq import physical_constants

__all__ = ['HarmonicTidalForcing', 'AtmosphericForcing', 'compute_wind_stress']


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


def wind_drag_coefficient(wind_mag, method='LargeYeager2009'):
    """C_D of the wind speed ``wind_mag`` by the three formulations of thetis/forcing.py:61-75, in the order of operations that
    ``swe_atm_drag`` (csrc/swe2d_atm.hip) repeats: the sixth power is ``m2 = m*m; m6 = m2*m2*m2``"""
    if method not in _lib.ATM_METHODS:
        raise ValueError("unknown wind stress method {!r}: one of {:}".format(method, sorted(_lib.ATM_METHODS)))
    m = np.asarray(wind_mag, dtype=np.float64)
    if method == 'LargePond1981':
        return np.where(m > 11.0, 1.0e-3*(0.49 + 0.065*m), 1.2e-3)
    if method == 'SmithBanke1975':
        return (0.63 + 0.066*m)/1000.
    m2 = m*m
    m6 = m2*m2*m2
    return np.where(m > 33.0, 2.34e-3, 1.e-3*(2.7/(m + 1e-3) + 0.142 + m/13.09 - 3.14807e-10*m6))


def compute_wind_stress(wind_u, wind_v, method='LargeYeager2009'):
    """Wind stress ``tau = C_D rho_air |U10| U10`` from the 10 m wind (thetis/forcing.py:19-79), by the formulations
    'LargeYeager2009' (default; C_D = 2.34e-3 above 33 m/s), 'LargePond1981' (switch at 11 m/s) or 'SmithBanke1975'.
    Returns (tau_x, tau_y) as arrays.

    The order of evaluation is fixed so that the device repeats it bit for bit (csrc/swe2d_atm.hip): the speed is
    ``sqrt(u*u + v*v)`` and its sixth power ``m2 = m*m; m6 = m2*m2*m2`` - the reference takes ``numpy.hypot`` and ``**6``, which
    differ from these at round-off -, everything else left to right as the reference writes it."""
    rho_air = float(physical_constants['rho_air'])
    u = np.asarray(wind_u, dtype=np.float64)
    v = np.asarray(wind_v, dtype=np.float64)
    m = np.sqrt(u*u + v*v)
    tau = wind_drag_coefficient(m, method)*rho_air*m
    return tau*u, tau*v


class AtmosphericForcing(object):
    RELTOL = 1e-6                   # slack on alpha outside [0, 1] (thetis/interpolation.py:819); within it alpha is clamped

    def __init__(self, wind_stress_field, atm_pressure_field, times, wind_u=None, wind_v=None, pressure=None,
                 method='LargeYeager2009', pressure_units='pa'):
        """
        :arg wind_stress_field: vector CG-P1 :class:`Function` that :meth:`set_fields` writes, or None: the wind is not forced
        :arg atm_pressure_field: scalar CG-P1 :class:`Function`, or None: the pressure is not forced
        :arg times: (n_t,) strictly increasing snapshot times in seconds of simulation time, n_t >= 2; the spacing may vary
        :arg wind_u, wind_v, pressure: (n_t, n_vertices) tables on the mesh vertices, in mesh coordinates (the tables of a quantity
            that is not forced may be None)
        :kwarg method: the stress formulation of :func:`compute_wind_stress`
        :kwarg pressure_units: 'pa' or 'hpa'; 'hpa' multiplies the pressure by 100 - here once, when the table is taken, so that the
            host and the device interpolate the same numbers
        The tables are copied: later changes of the arrays handed in are not seen.  No file readers, no regridding, no rotation.
        """
        if wind_stress_field is None and atm_pressure_field is None:
            raise ValueError('at least one of wind_stress_field and atm_pressure_field is required')
        if method not in _lib.ATM_METHODS:
            raise ValueError("unknown wind stress method {!r}: one of {:}".format(method, sorted(_lib.ATM_METHODS)))
        if pressure_units not in ('pa', 'hpa'):
            raise ValueError("pressure_units must be 'pa' or 'hpa'")
        mesh = None
        for f, vector, what in ((wind_stress_field, True, 'wind_stress_field'), (atm_pressure_field, False, 'atm_pressure_field')):
            if f is None:
                continue
            if not isinstance(f, Function):
                raise ValueError('{:} must be a Function or None'.format(what))
            fs = f.function_space()
            if fs.family != 'CG' or fs.degree != 1 or bool(fs.vector) != vector:
                raise ValueError('{:} must be a {:} CG-P1 Function'.format(what, 'vector' if vector else 'scalar'))
            if mesh is not None and fs.mesh() is not mesh:
                raise ValueError('wind_stress_field and atm_pressure_field live on different meshes')
            mesh = fs.mesh()
        self.mesh = mesh
        self.wind_stress_field = wind_stress_field
        self.atm_pressure_field = atm_pressure_field
        self.method = method
        self.pressure_units = pressure_units
        self.times = np.array(times, dtype=np.float64).reshape(-1)
        n_t, n_v = len(self.times), mesh.num_vertices
        if n_t < 2:
            raise ValueError('at least two snapshot times are required')
        if not np.isfinite(self.times).all() or not (np.diff(self.times) > 0.0).all():
            raise ValueError('times must be finite and strictly increasing')

        def table(a, what):
            if a is None:
                raise ValueError('{:} is required'.format(what))
            a = np.array(a, dtype=np.float64)
            if a.shape != (n_t, n_v):
                raise ValueError('{:} must have shape (n_t, n_vertices) = ({:d}, {:d}), got {:}'.format(what, n_t, n_v, a.shape))
            if not np.isfinite(a).all():
                raise ValueError('{:} must be finite'.format(what))
            return a
        self.wind_u = self.wind_v = self.pressure = None
        if wind_stress_field is not None:
            self.wind_u, self.wind_v = table(wind_u, 'wind_u'), table(wind_v, 'wind_v')
        if atm_pressure_field is not None:
            self.pressure = table(pressure, 'pressure')
            if pressure_units == 'hpa':
                self.pressure = self.pressure*100

    @property
    def which(self):
        """the quantities forced: include/swe2d.h SWE2D_ATM_WIND | SWE2D_ATM_PRESSURE"""
        return (_lib.ATM_WIND if self.wind_stress_field is not None else 0) | (_lib.ATM_PRESSURE if self.atm_pressure_field is not None else 0)

    def table_signature(self):
        """what the device's copy of the record was made from (the tables are copied at construction and never change)"""
        return (id(self), self.method, self.which, len(self.times))

    def bracket(self, t):
        """(j, alpha): the snapshots j, j + 1 that bracket ``t`` - j the largest index with times[j] <= t, at most n_t - 2 - and the
        weight of the later one; the arithmetic of ``atm_bracket`` in csrc/swe2d_atm.hip"""
        t = float(t)
        tm = self.times
        j = min(max(int(np.searchsorted(tm, t, side='right')) - 1, 0), len(tm) - 2)
        alpha = (t - float(tm[j]))/(float(tm[j + 1]) - float(tm[j]))
        if not (alpha >= -self.RELTOL and alpha <= 1.0 + self.RELTOL):
            raise ValueError('time t = {!r} is outside the atmospheric record [{!r}, {!r}]'.format(t, float(tm[0]), float(tm[-1])))
        return j, min(max(alpha, 0.0), 1.0)

    def evaluate(self, t):
        """(tau_x, tau_y, p) per vertex at time ``t`` (None for a quantity that is not forced) - THE expression of every host path"""
        j, alpha = self.bracket(t)

        def interp(a):
            return (1.0 - alpha)*a[j] + alpha*a[j + 1]
        tx = ty = p = None
        if self.wind_u is not None:
            tx, ty = compute_wind_stress(interp(self.wind_u), interp(self.wind_v), method=self.method)
        if self.pressure is not None:
            p = interp(self.pressure)
        return tx, ty, p

    def set_fields(self, t):
        """writes the wind stress and the pressure of time ``t`` into the two fields (thetis/forcing.py:148)"""
        tx, ty, p = self.evaluate(t)
        if tx is not None:
            d = self.wind_stress_field.dat.data          # (a writable view: the field's host version moves on)
            d[:, 0] = tx
            d[:, 1] = ty
        if p is not None:
            self.atm_pressure_field.dat.data[...] = p
