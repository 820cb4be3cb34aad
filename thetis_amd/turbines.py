"""
Tidal turbine farms (thetis/turbines.py:17-171, 213-264): turbine types, ``TidalTurbineFarm`` and ``TurbineFunctionalCallback``.

The drag term and the power integral are evaluated on the device (csrc/swe2d_kernels.h: swe_farm_terms, csrc/swe2d_turbine.hip:
swe_turbine_power_kernel); the classes here hold the parameters, state the same formulas in numpy for host-side use
(``friction_coefficient``, ``number_of_turbines``) and hand the device what it needs (``device_params``, ``density_nodal``).
``DiscreteTidalTurbineFarm`` (turbines.py:174-210) places single turbines as bump densities; its drag is a pass of its own after
each stage launch and its power, per farm and per turbine, is integrated with the farm's own rule (csrc/swe2d_dfarm.hip).
Not here: the pyadjoint half of the reference's module (optimisation callback, distance constraints), moving turbines and the
shear profile - each raises ``NotImplementedError`` naming the option.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib
from .callback import DiagnosticCallback
from .function import Function, cell_quadrature, farm_quadrature
from .options import Constant
from .shallowwater_eq import physical_constants

__all__ = ['TidalTurbine', 'ConstantThrustTurbine', 'TabulatedThrustTurbine', 'TidalTurbineFarm', 'DiscreteTidalTurbineFarm',
           'TurbineFunctionalCallback', 'linearly_interpolate_table', 'farm_cells', 'build_farms', 'BUMP_NORM']


def linearly_interpolate_table(x_list, y_list, y_final, x):
    """y(x) of a table for x >= x_list[0]: linear between entries, ``y_final`` from x_list[-1] on (turbines.py:109-125)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape, float(y_final))
    for j in range(len(x_list) - 2, -1, -1):
        x0, x1, y0, y1 = x_list[j], x_list[j + 1], y_list[j], y_list[j + 1]
        out = np.where(x < x1, ((x1 - x)*y0 + (x - x0)*y1)/(x1 - x0), out)
    return out


class TidalTurbine(object):
    """turbines.py:17-93 without the shear profile"""

    def __init__(self, options, upwind_correction=False):
        if options.apply_shear_profile:
            raise NotImplementedError('apply_shear_profile=True (rotor-averaged velocity of a sheared profile) is not implemented on '
                                      'the device path')
        self.diameter = options.diameter
        self.projected_diameter = options.projected_diameter or self.diameter
        self.C_support = options.C_support
        self.A_support = options.A_support
        self.upwind_correction = bool(upwind_correction)
        self.apply_shear_profile = False

    @property
    def rotor_area(self):
        return math.pi*self.diameter**2/4

    @staticmethod
    def _speed(uv):
        uv = np.asarray(uv, dtype=np.float64)
        return np.sqrt(uv[..., 0]**2 + uv[..., 1]**2)

    def _thrust_area(self, uv):
        fric = self.thrust_coefficient(uv)*self.rotor_area
        if self.C_support:
            fric = fric + self.C_support*self.A_support
        return fric

    def velocity_correction(self, uv, depth):
        if self.upwind_correction:
            return 0.5*(1 + np.sqrt(1 - self._thrust_area(uv)/(self.projected_diameter*np.asarray(depth))))
        return 1

    def friction_coefficient(self, uv, depth):
        return self._thrust_area(uv)/2./self.velocity_correction(uv, depth)**2

    def power(self, uv, depth):
        alpha = self.velocity_correction(uv, depth)
        uv3 = self._speed(uv)**3/alpha**3
        speed = np.cbrt(uv3)
        c_p = self.power_coefficient(np.stack([speed, np.zeros_like(speed)], axis=-1))
        return 0.5*float(physical_constants['rho0'])*self.rotor_area*c_p*uv3


class ConstantThrustTurbine(TidalTurbine):
    def __init__(self, options, upwind_correction=False):
        super().__init__(options, upwind_correction=upwind_correction)
        self.C_T = options.thrust_coefficient
        self.C_P = options.power_coefficient or 0.5*self.C_T*(1 + (1 - self.C_T)**0.5)

    def thrust_coefficient(self, uv):
        return self.C_T

    def power_coefficient(self, uv):
        return self.C_P


class TabulatedThrustTurbine(TidalTurbine):
    def __init__(self, options, upwind_correction=False):
        super().__init__(options, upwind_correction=upwind_correction)
        self.C_T = list(options.thrust_coefficients)
        self.C_P = list(options.power_coefficients or [0.5*c_t*(1 + (1 - c_t)**0.5) for c_t in self.C_T])
        self.speeds = list(options.thrust_speeds)
        if not len(self.C_T) == len(self.speeds):
            raise ValueError("In tabulated thrust curve the number of thrust coefficients and speed values should be the same.")
        if not len(self.C_P) == len(self.speeds):
            raise ValueError("In tabulated thrust curve the number of power coefficients and speed values should be the same.")
        if len(self.speeds) < 2 or len(self.speeds) > _lib.MAX_THRUST_TABLE:
            raise NotImplementedError('thrust_speeds: a thrust table has 2 .. SWE2D_MAX_THRUST_TABLE = {:d} entries on the device '
                                      'path (got {:d})'.format(_lib.MAX_THRUST_TABLE, len(self.speeds)))
        if np.any(np.diff(self.speeds) <= 0):
            raise ValueError('thrust_speeds must increase strictly')

    def _table(self, y, uv):
        umag = self._speed(uv)
        return np.where(umag < self.speeds[0], 0.0, linearly_interpolate_table(self.speeds, y, 0, umag))

    def thrust_coefficient(self, uv):
        return self._table(self.C_T, uv)

    def power_coefficient(self, uv):
        return self._table(self.C_P, uv)


def farm_cells(mesh, subdomain):
    """bool (N,): the cells ``dx(subdomain)`` covers - those with ``cell_markers == subdomain``, or all for 'everywhere'"""
    if isinstance(subdomain, str):
        if subdomain != 'everywhere':
            raise ValueError("a farm's subdomain is a cell marker or 'everywhere', not {!r}".format(subdomain))
        return np.ones(mesh.num_cells, dtype=bool)
    markers = getattr(mesh, 'cell_markers', None)
    if markers is None:
        markers = np.zeros(mesh.num_cells, dtype=np.int32)
    mask = np.asarray(markers) == int(subdomain)
    if not mask.any():
        raise ValueError('tidal_turbine_farms: no cell of the mesh has the subdomain id {!r}'.format(subdomain))
    return mask


def _integrate_cells(mesh, nodal):
    """per cell: int f dx of nodal P1 / Q1 values (N, k), by the rule of the drag term"""
    p = mesh.cell_xy()
    phi, w = cell_quadrature(p.shape[1])
    fq = nodal @ phi.T                                           # (N, q)
    if p.shape[1] == 3:
        return mesh.cell_areas()*(fq @ w)
    a, b = p[:, 1] - p[:, 0], p[:, 3] - p[:, 0]
    c = p[:, 0] - p[:, 1] + p[:, 2] - p[:, 3]
    cross = lambda s, t: s[:, 0]*t[:, 1] - s[:, 1]*t[:, 0]       # noqa: E731
    d0, d1, d2 = cross(a, b), cross(a, c), cross(c, b)
    # the rule's points in (xi, zeta): phi = ((1-xi)(1-ze), xi(1-ze), xi ze, (1-xi) ze)
    xi, ze = phi[:, 1] + phi[:, 2], phi[:, 2] + phi[:, 3]
    return ((d0[:, None] + d1[:, None]*xi + d2[:, None]*ze)*fq) @ w


class TidalTurbineFarm(object):
    """turbines.py:148-171.  ``dx`` of the reference is the farm's subdomain here (a cell marker or 'everywhere')."""

    def __init__(self, turbine_density, subdomain, options, mesh):
        upwind_correction = getattr(options, 'upwind_correction', False)
        if options.turbine_type == 'constant':
            self.turbine = ConstantThrustTurbine(options.turbine_options, upwind_correction=upwind_correction)
        elif options.turbine_type == 'table':
            self.turbine = TabulatedThrustTurbine(options.turbine_options, upwind_correction=upwind_correction)
        self.subdomain = subdomain
        self.dx = subdomain
        self.mesh = mesh
        self.cells = farm_cells(mesh, subdomain)
        self.turbine_density = turbine_density
        self.break_even_wattage = options.break_even_wattage
        self._solver = None
        self._index = None

    def density_signature(self):
        d = self.turbine_density
        if isinstance(d, Function):
            return ('f', id(d), d._host_version)
        return ('c', float(d))

    def density_nodal(self):
        """(N, k) DG nodal values of the density, zero outside the farm's cells (a CG density's taper beyond the farm contributes
        nothing, as ``dx(subdomain)`` in the reference)"""
        d = self.turbine_density
        mesh = self.mesh
        k = mesh.cells.shape[1]
        if isinstance(d, Function):
            fs = d.function_space()
            if fs.vector or fs.degree != 1:
                raise NotImplementedError('turbine_density must be a Constant or a CG-P1 / DG-P1 Function')
            vals = np.array(d.cell_node_values(), dtype=np.float64).reshape(mesh.num_cells, k)
        elif callable(d):
            raise NotImplementedError('turbine_density must be a Constant or a CG-P1 / DG-P1 Function')
        else:
            vals = np.full((mesh.num_cells, k), float(d))
        vals = np.where(self.cells[:, None], vals, 0.0)
        if not np.all(vals >= 0.0):
            raise ValueError('turbine_density must be >= 0')
        return np.ascontiguousarray(vals)

    def number_of_turbines(self):
        return float(_integrate_cells(self.mesh, self.density_nodal()).sum())

    def friction_coefficient(self, uv, depth):
        return self.turbine.friction_coefficient(uv, depth)

    def power_output(self, uv=None, depth=None):
        """int power * density dx of the solver's current state, on the device (the arguments of the reference's method - the
        solution's velocity and the static bathymetry - are what the kernel reads)."""
        if self._solver is None:
            raise RuntimeError('the farm is not attached to a solver (FlowSolver2d.create_equations builds the farms)')
        return float(_swe_stepper(self._solver).turbine_power()[self._index])

    def device_params(self):
        """swe2d_turbine_params of this farm"""
        t = self.turbine
        p = _lib.TurbineParams()
        p.support_area = t.C_support*t.A_support if t.C_support else 0.0
        p.rotor_area = t.rotor_area
        p.projected_diameter = t.projected_diameter
        p.upwind_correction = int(t.upwind_correction)
        p.rho0 = float(physical_constants['rho0'])
        if isinstance(t, TabulatedThrustTurbine):
            p.n_table = len(t.speeds)
            for j in range(p.n_table):
                p.speeds[j], p.thrust[j], p.power[j] = t.speeds[j], t.C_T[j], t.C_P[j]
        else:
            p.n_table = 0
            p.thrust_area_const = t.C_T*t.rotor_area
            p.power_const = t.C_P
        return p


BUMP_NORM = 1.45661      # integral of the unit bump over its square, as the reference rounds it (turbines.py:210)


def _bump(s):
    """psi(s) = exp(1 - 1/(1 - s^2)) inside |s| < 1, zero at and beyond (turbines.py:201-208)"""
    s = np.asarray(s, dtype=np.float64)
    inside = np.abs(s) < 1.0
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        return np.where(inside, np.exp(1.0 - 1.0/(1.0 - np.where(inside, s, 0.0)**2)), 0.0)


class DiscreteTidalTurbineFarm(TidalTurbineFarm):
    """turbines.py:174-210: turbines at coordinates, each a bump of radius projected_diameter/2 that integrates to one turbine.
    The density is not a Function here: the device tabulates it at the points of the farm's rule (``quadrature_degree``,
    function.farm_quadrature) in the cells around the turbines, ``turbine_density`` states the same sum in numpy."""

    def __init__(self, mesh, subdomain, options):
        super().__init__(None, subdomain, options, mesh)
        self.quadrature_degree = int(options.quadrature_degree)
        self.phi, self.w = farm_quadrature(mesh.cells.shape[1], self.quadrature_degree)
        self.radius = 0.5*self.turbine.projected_diameter
        self.coordinates = np.zeros((0, 2))
        self.turbine_density = self.density
        self.add_turbines(options.turbine_coordinates)

    def add_turbines(self, coordinates):
        """append turbines at ``coordinates``: pairs of floats or ``Constant``s (turbines.py:189-199)"""
        xy = np.array([[float(c) for c in pair] for pair in coordinates], dtype=np.float64).reshape(-1, 2)
        if not np.isfinite(xy).all():
            raise ValueError('turbine_coordinates must be finite')
        self.coordinates = np.concatenate([self.coordinates, xy])

    def density(self, xy):
        """the bump sum at points ``xy`` (..., 2), turbine after turbine"""
        xy = np.asarray(xy, dtype=np.float64)
        r = self.radius
        d = np.zeros(xy.shape[:-1])
        for x_t, y_t in self.coordinates:
            d = d + _bump((xy[..., 0] - x_t)/r)*_bump((xy[..., 1] - y_t)/r)/(r**2*BUMP_NORM)
        return d

    def density_signature(self):
        return ('d', self.coordinates.tobytes(), self.quadrature_degree, self.radius)

    def density_nodal(self):
        raise NotImplementedError('a discrete farm has no nodal density: its bumps are tabulated at the points of its own rule')

    def _cell_points(self):
        """(N, q, 2) the rule's points in every cell (left to right, as the device forms them), (N, q) weight * det J"""
        p = self.mesh.cell_xy()
        pts = self.phi[None, :, 0, None]*p[:, None, 0, :]
        for i in range(1, p.shape[1]):
            pts = pts + self.phi[None, :, i, None]*p[:, None, i, :]
        if p.shape[1] == 3:
            jac = self.mesh.cell_areas()[:, None]*np.ones(len(self.w))
        else:
            a, b = p[:, 1] - p[:, 0], p[:, 3] - p[:, 0]
            c = p[:, 0] - p[:, 1] + p[:, 2] - p[:, 3]
            cross = lambda s, t: s[:, 0]*t[:, 1] - s[:, 1]*t[:, 0]       # noqa: E731
            xi, ze = self.phi[:, 1] + self.phi[:, 2], self.phi[:, 2] + self.phi[:, 3]
            jac = cross(a, b)[:, None] + cross(a, c)[:, None]*xi + cross(c, b)[:, None]*ze
        return pts, jac*self.w

    def number_of_turbines(self):
        """int density dx(subdomain) with the farm's rule (close to, not exactly, the number of turbines placed: the bump is not a
        polynomial, its norm has five digits, and a bump may reach beyond the subdomain)"""
        pts, wj = self._cell_points()
        return float((self.density(pts)*wj)[self.cells].sum())

    def turbine_powers(self):
        """power of every turbine, of the solver's current state, on the device"""
        if self._solver is None:
            raise RuntimeError('the farm is not attached to a solver (FlowSolver2d.create_equations builds the farms)')
        stepper = _swe_stepper(self._solver)
        stepper._sync_to_device()
        return stepper.device.dfarm_turbine_power(self._index)


def _swe_stepper(solver_obj):
    stepper = solver_obj.timestepper
    return getattr(stepper, 'swe', stepper)            # the coupled integrator (tracers) holds the shallow water stepper


def build_farms(options, mesh):
    """``FlowSolver2d.tidal_farms``: the list of farms in the reference's order (solver2d.py:462-485), or None"""
    if len(options.tidal_turbine_farms) + len(options.discrete_tidal_turbine_farms) == 0:
        return None
    farms = []
    for subdomain, farm_options_list in options.tidal_turbine_farms.items():
        if not isinstance(farm_options_list, list):
            raise TypeError('Farm options must be entered as a list e.g. '
                            'solver2d.FlowSolver2d(mesh2d, bathymetry_2d).options.tidal_turbine_farms[site_ID] = [farm_options]')
        for farm_options in farm_options_list:
            farms.append(TidalTurbineFarm(farm_options.turbine_density, subdomain, farm_options, mesh))
    for subdomain, farm_options_list in options.discrete_tidal_turbine_farms.items():
        if not isinstance(farm_options_list, list):
            raise TypeError('Farm options must be entered as a list e.g. '
                            'solver2d.FlowSolver2d(mesh2d, bathymetry_2d).options.discrete_tidal_turbine_farms[site_ID] = [farm_options]')
        if farm_options_list and getattr(options, 'use_wetting_and_drying', False):
            raise NotImplementedError('discrete_tidal_turbine_farms with use_wetting_and_drying: the discrete farms\' pass does not '
                                      'carry the wetting-drying depth')
        for farm_options in farm_options_list:
            farm = DiscreteTidalTurbineFarm(mesh, subdomain, farm_options)
            if len(farm.coordinates) == 0:
                # (the reference builds such a farm for its optimisation workflow, which places and moves the turbines later)
                raise NotImplementedError('discrete_tidal_turbine_farms: a farm without turbine_coordinates - turbines placed or '
                                          'moved after the equations are built belong to the optimisation workflow, which is not '
                                          'on the device path; give the coordinates in DiscreteTidalTurbineFarmOptions')
            farms.append(farm)
    if len(farms) > _lib.MAX_FARMS:
        raise NotImplementedError('tidal_turbine_farms: more than SWE2D_MAX_FARMS = {:d} farms (continuous and discrete '
                                  'together)'.format(_lib.MAX_FARMS))
    return farms


class TurbineFunctionalCallback(DiagnosticCallback):
    """:class:`.DiagnosticCallback` that evaluates the performance of each tidal turbine farm (turbines.py:213-264).  Registered
    with 'timestep' it keeps ``FlowSolver2d.iterate`` batching its steps: the device appends one power row per step
    (``row_probe``), the host integrates the rows after the batch in step order (``take_row``) - the values of stepping one by one."""

    name = 'turbine'
    variable_names = ['current_power', 'average_power', 'average_profit']

    def __init__(self, solver_obj, **kwargs):
        if not hasattr(solver_obj, 'tidal_farms'):
            solver_obj.create_equations()
        self.farms = solver_obj.tidal_farms
        if not self.farms:
            raise ValueError('TurbineFunctionalCallback: the solver has no tidal_turbine_farms')
        nfarms = len(self.farms)
        self.export_to_hdf5 = kwargs.pop('export_to_hdf5', False)
        self.outputdir = kwargs.pop('outputdir', None)
        super().__init__(solver_obj, **kwargs)
        self.dt = solver_obj.options.timestep
        self.cost = [farm.number_of_turbines() for farm in self.farms]
        if self.append_to_log:
            from .log import print_output
            print_output('Number of turbines = {}'.format(sum(self.cost)))
        self.break_even_wattage = [farm.break_even_wattage for farm in self.farms]
        self.instantaneous_power = [0]*nfarms
        self.integrated_power = [0]*nfarms
        self.average_power = [0]*nfarms
        self.average_profit = [0]*nfarms
        self.time_period = 0.

    def _integrate(self, powers):
        """Perform time integration and return current power and time-averaged power and profit."""
        dt = self.solver_obj.dt if self.solver_obj.dt is not None else self.dt
        self.time_period = self.time_period + dt
        current_power = []
        for i in range(len(self.farms)):
            power = float(powers[i])
            current_power.append(power)
            self.instantaneous_power[i] = power
            self.integrated_power[i] += power*dt
            self.average_power[i] = self.integrated_power[i]/self.time_period
            self.average_profit[i] = self.average_power[i] - self.break_even_wattage[i]*self.cost[i]
        return current_power, list(self.average_power), list(self.average_profit)

    def __call__(self):
        return self._integrate(_swe_stepper(self.solver_obj).turbine_power())

    def message_str(self, current_power, average_power, average_profit):
        return 'Current power, average power and profit for each farm: {}, {}, {}'.format(current_power, average_power, average_profit)

    # ---- rows of a batch (FlowSolver2d.create_iterator)
    def row_probe(self, n_rows):
        from .pointeval import device_ready
        stepper = _swe_stepper(self.solver_obj)
        dev = getattr(stepper, 'device', None)
        if dev is None or not hasattr(dev, 'turbine_rows_reserve') or not device_ready(stepper):
            return None
        dev.turbine_rows_reserve(n_rows)
        return dev, dev.TURBINE_ROWS

    def take_row(self, t, values):
        if t < self.start_time or t > self.end_time:
            return
        out = self._integrate(values)
        self.history.append((t,) + out)
        if self.append_to_log:
            self.push_to_log(t, out)

    def export(self):
        """rank 0 rewrites diagnostic_turbine.npz with the history so far (the detectors' substitute for the HDF5 file)"""
        if not self.export_to_hdf5 or getattr(self.solver_obj.comm, 'rank', 0) != 0:
            return
        outdir = self.outputdir or self.solver_obj.options.output_directory
        os.makedirs(outdir, exist_ok=True)
        n = len(self.history)
        data = {'time': np.array([h[0] for h in self.history], dtype=np.float64).reshape(n, 1)}
        for j, vn in enumerate(self.variable_names):
            data[vn] = np.array([h[1 + j] for h in self.history], dtype=np.float64).reshape(n, len(self.farms))
        path = os.path.join(outdir, 'diagnostic_{:}.npz'.format(self.name))
        tmp = path + '.tmp.npz'
        np.savez(tmp, **data)
        os.replace(tmp, path)
