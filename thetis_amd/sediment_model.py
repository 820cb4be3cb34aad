"""
Sediment model: the closures of the reference's ``thetis/sediment_model.py`` for the suspended load - critical Shields parameter,
settling velocity, bed friction, Rouse profile, erosion and deposition - and the Exner source term.

This build's formulation.  The reference projects ``uv`` and the total depth into CG-P1 with a global solve and
interpolates the closures there.  Here they are evaluated at the DG nodes of each cell from that cell's own nodal ``uv`` and
``H = eta + h``; the erosion and deposition terms of the sediment equation are interpolated at the nodes, not projected; the
Exner equation is advanced in its lumped-mass CG-P1 form.  The device passes are in ``csrc/swe2d_sediment.hip``;
:class:`HostSediment` restates them in numpy - the replay the tests compare against, and what the sediment stepper
(``coupled_timeintegrator_2d._SedimentStepper``) evaluates per stage for a device class without the sediment calls.
"""
import numpy as np

from .function import Function
from .log import print_output
from .options import Constant

__all__ = ['SedimentModel', 'SedimentEquation2D', 'HostSediment', 'sediment_constants', 'closures', 'check_sediment_options', 'device_parameters',
           'EXNER_MIN_DEPTH']

EXNER_MIN_DEPTH = 1e-3       # a vertex whose depth an Exner update would take below this keeps its bed (and is counted)


def _thetacr(dstar):
    """critical Shields parameter (sediment_model.py:142-145)"""
    if dstar < 4:
        return 0.24*dstar**(-1)
    if dstar < 10:
        return 0.14*dstar**(-0.64)
    if dstar < 20:
        return 0.04*dstar**(-0.1)
    if dstar < 150:
        return 0.013*dstar**0.29
    return 0.055


def _settling_velocity(d, R, g, nu):
    """sediment_model.py:151-155"""
    if d <= 1e-04:
        return g*(d**2)*R/(18*nu)
    if d <= 1e-03:
        return (10*nu/d)*(np.sqrt(1 + 0.01*((R*g*(d**3))/(nu**2))) - 1)
    return 1.1*np.sqrt(g*d*R)


def sediment_constants(average_size, bed_reference_height, viscosity, sediment_density=2650.0, rho0=1000.0, g=9.81, kappa=0.4,
                       porosity=0.4, morfac=1.0):
    """The constants of a run (sediment_model.py:121-155): every quantity that depends on the grain and the fluid only."""
    d, ks, nu, rhos = float(average_size), float(bed_reference_height), float(viscosity), float(sediment_density)
    R = rhos/rho0 - 1
    dstar = d*((g*R)/(nu**2))**(1/3)
    if dstar < 1:
        raise ValueError('dstar value less than 1')
    thetacr = _thetacr(dstar)
    a = ks/2
    c = dict(average_size=d, R=R, dstar=dstar, thetacr=thetacr, taucr=(rhos - rho0)*g*d*thetacr,
             ws=float(_settling_velocity(d, R, g, nu)), a=a, ksp=3*d, ks=ks, rho0=float(rho0), g=float(g), kappa=float(kappa),
             fac=float(morfac)/(1 - float(porosity)))
    c['erosion_factor'] = 0.015*(d/a)/(dstar**0.3)
    return c


def closures(c, u, v, H):
    """The flow-dependent closures (sediment_model.py:165-211) at points with velocity (u, v) and total depth H: numpy arrays of
    one shape.  Every conditional is a select and no logarithm, power or root sees an argument outside its domain on any branch -
    operation by operation what swe_sediment_closures does on the device."""
    u, v, H = (np.asarray(x, dtype=np.float64) for x in (u, v, H))
    kappa, ws, ks, ksp, a = c['kappa'], c['ws'], c['ks'], c['ksp'], c['a']
    with np.errstate(divide='ignore'):
        unorm = u*u + v*v
        hc = np.where(H > 0.001, H, 0.001)
        ax = 11.036*hc/ks
        aux = np.where(ax > 1.001, ax, 1.001)
        lq = np.log(aux)/kappa
        qfc = 2.0/(lq*lq)
        deep = H > ksp
        lc = (1.0/kappa)*np.log(11.036*np.where(deep, H, ksp)/ksp)
        cfactor = np.where(deep, 2.0/(lc*lc), 0.0)
        mu = np.where(qfc > 0.0, cfactor/qfc, 0.0)
        B = np.where(a > H, 1.0, a/np.where(a > H, 1.0, H))
        ustar = np.sqrt(0.5*qfc*unorm)
        rouse = ws/(kappa*ustar) - 1.0
        rm = np.where(rouse < 3.0, rouse, 3.0)
        power = np.abs(rouse) > 1e-4
        rms = np.where(power, rm, 1.0)
        step = np.where(power, B*(1.0 - np.power(B, rms))/rms, -B*np.log(B))
        ir0 = np.where(step > 1e-12, 1.0/np.where(step > 1e-12, step, 1.0), 1e12)
        integrated_rouse = np.where(ir0 > 1.0, ir0, 1.0)
        tau = c['rho0']*0.5*qfc*unorm*mu
        T = np.where(tau > 0.0, (tau - c['taucr'])/c['taucr'], -1.0)
        T15 = np.where(T > 0.0, T*np.sqrt(np.where(T > 0.0, T, 0.0)), 0.0)
        erosion_concentration = c['erosion_factor']*T15
        E = ws*erosion_concentration
        D = ws*integrated_rouse
    return dict(qfc=qfc, cfactor=cfactor, mu=mu, B=B, ustar=ustar, rouse_number=rouse, intermediate_step=step,
                integrated_rouse=integrated_rouse, transport_stage_param=T, erosion_concentration=erosion_concentration,
                erosion=E, deposition=D, equilibrium=E/D)


def device_parameters(c, conservative=False, solve_exner=False, min_depth=EXNER_MIN_DEPTH):
    """``sediment_constants`` -> the fields of include/swe2d.h swe2d_sediment_params"""
    p = {k: c[k] for k in ('ws', 'dstar', 'taucr', 'a', 'ksp', 'ks', 'rho0', 'kappa', 'fac', 'erosion_factor')}
    p.update(min_depth=float(min_depth), conservative=int(bool(conservative)), solve_exner=int(bool(solve_exner)))
    return p


class HostSediment(object):
    """The four device passes in numpy on a triangle mesh: ``cells`` (N, 3), ``vertex_xy`` (V, 2).  Given the same planes the
    source, the 'equilibrium' table and the Exner update have the bits of the device (+ - * / in the same order); the
    coefficient planes agree to the rounding of the two math libraries."""

    def __init__(self, cells, vertex_xy, constants, conservative=False, nonlinear=True, min_depth=EXNER_MIN_DEPTH):
        self.cells = np.asarray(cells, dtype=np.int64)
        if self.cells.ndim != 2 or self.cells.shape[1] != 3:
            raise NotImplementedError('the sediment model runs on triangles only')
        xy = np.asarray(vertex_xy, dtype=np.float64)
        self.c = dict(constants)
        self.conservative, self.nonlinear, self.min_depth = bool(conservative), bool(nonlinear), float(min_depth)
        x, y = xy[self.cells, 0], xy[self.cells, 1]
        p = (x[:, 1] - x[:, 0])*(y[:, 2] - y[:, 0])
        q = (x[:, 2] - x[:, 0])*(y[:, 1] - y[:, 0])
        self.area = 0.5*np.abs(p - q)
        self.n_vertices = xy.shape[0]
        # vertex -> (cell, local node), cells ascending
        flat = self.cells.reshape(-1)
        order = np.argsort(flat, kind='stable')
        self.v_cell, self.v_node = order//3, order % 3
        self.v_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=self.n_vertices))])
        self.n_skipped = 0

    def depth(self, eta, bath):
        h = np.asarray(bath, dtype=np.float64)[self.cells]
        return np.asarray(eta, dtype=np.float64) + h if self.nonlinear else h

    def coefficients(self, uv, eta, bath):
        """(E, D, equilibrium), each (N, 3), from nodal ``uv`` (N, 3, 2), ``eta`` (N, 3) and the vertex bathymetry"""
        uv = np.asarray(uv, dtype=np.float64)
        out = closures(self.c, uv[..., 0], uv[..., 1], self.depth(eta, bath))
        return out['erosion'], out['deposition'], out['equilibrium']

    def net_erosion(self, E, D, S, eta, bath):
        """r = E - D*S at the nodes (conservative: E - (D*q)/H): the Exner source and H times the sediment source"""
        if self.conservative:
            return E - (D*S)/self.depth(eta, bath)
        return E - D*S

    def source(self, E, D, S, eta, bath):
        """nodal source of the sediment tracer for a stage whose input is ``S``"""
        if self.conservative:
            return E - (D*S)/self.depth(eta, bath)
        return (E - D*S)/self.depth(eta, bath)

    def boundary_values(self, equilibrium, eta, bath):
        """what the 'equilibrium' facets of the per-facet value table hold at the nodes of a cell"""
        return equilibrium*self.depth(eta, bath) if self.conservative else equilibrium

    def exner(self, E, D, S, eta, bath, dt):
        """one bed update: the new vertex bathymetry (vertices whose depth would fall below the floor keep theirs)"""
        bath = np.asarray(bath, dtype=np.float64)
        r = self.net_erosion(E, D, S, eta, bath)
        dtf = dt*self.c['fac']
        w12, w3 = self.area/12.0, self.area/3.0
        eta = np.asarray(eta, dtype=np.float64)
        # per (vertex, cell) entry in list order; np.add.at accumulates the entries of a vertex one after the other in that order,
        # which is the device's loop
        k, i = self.v_cell, self.v_node
        vert = np.repeat(np.arange(self.n_vertices), np.diff(self.v_off))
        contrib = w12[k]*((2.0*r[k, i] + r[k, (i + 1) % 3]) + r[k, (i + 2) % 3])
        num, den = np.zeros(self.n_vertices), np.zeros(self.n_vertices)
        np.add.at(num, vert, contrib)
        np.add.at(den, vert, w3[k])
        eta_min = np.full(self.n_vertices, 1e300)
        np.minimum.at(eta_min, vert, eta[k, i])
        used = den > 0.0
        b = bath + (dtf*num)/np.where(used, den, 1.0)
        ok = used & ((eta_min + b if self.nonlinear else b) >= self.min_depth)
        self.n_skipped += int((used & ~ok).sum())
        new = np.where(ok, b, bath)
        return new


def _constant_value(name, v):
    """a Constant / number of the sediment options; Functions and expressions are not on this path"""
    if isinstance(v, (int, float, np.floating, Constant)):
        return float(v)
    raise NotImplementedError('sediment_model_options.{:} must be a Constant on the device path (a spatially varying value '
                              'is not implemented)'.format(name))


def check_sediment_options(options, mesh2d=None, comm=None, tidal_farms=False):
    """What this build refuses of the sediment options, each by the option's name; returns the run's constants
    (``sediment_constants``).  Called when the equations are built."""
    from .shallowwater_eq import physical_constants
    so = options.sediment_model_options
    for name in ('use_bedload', 'use_sediment_slide', 'use_secondary_current'):
        if getattr(so, name):
            raise NotImplementedError('sediment_model_options.{:} is not implemented: this build runs the suspended load only '
                                      '(bedload, slide and secondary current differentiate the bed)'.format(name))
    if so.solve_suspended_sediment and so.use_advective_velocity_correction:
        raise NotImplementedError('sediment_model_options.use_advective_velocity_correction=True is not implemented (the tracer '
                                  'kernels take a scalar velocity factor): set it False')
    if so.solve_exner and not so.solve_suspended_sediment:
        raise NotImplementedError('sediment_model_options.solve_exner without solve_suspended_sediment has no source on this path '
                                  '(use_bedload is not implemented)')
    if options.use_wetting_and_drying:
        raise NotImplementedError('sediment_model_options.solve_suspended_sediment / solve_exner with use_wetting_and_drying is not '
                                  'implemented: the sediment kernels take H = eta + h, not the wetting-drying depth, and the depth '
                                  'planes of the explicit wetting-drying are tied to the bed')
    if mesh2d is not None and int(np.asarray(mesh2d.cells).shape[1]) != 3:
        raise NotImplementedError('sediment_model_options: the sediment model runs on triangles only (quadrilaterals are not implemented)')
    if comm is not None and getattr(comm, 'size', 1) > 1:
        raise NotImplementedError('sediment_model_options: the sediment model is not available on several ranks')
    if so.solve_exner and tidal_farms:
        raise NotImplementedError('sediment_model_options.solve_exner together with tidal turbine farms is not implemented')
    for name in ('sediment_timestepper_type', 'exner_timestepper_type'):
        active = so.solve_suspended_sediment if name.startswith('sediment') else so.solve_exner
        if active and getattr(so, name) not in ('SSPRK33', 'ForwardEuler'):
            raise NotImplementedError("sediment_model_options.{:}={!r}: the device path runs the explicit steppers 'SSPRK33' and "
                                      "'ForwardEuler' only".format(name, getattr(so, name)))
    if so.average_sediment_size is None:
        raise ValueError('sediment_model_options.average_sediment_size is not set')
    if so.bed_reference_height is None:
        raise ValueError('sediment_model_options.bed_reference_height is not set')
    nu = so.morphological_viscosity if so.morphological_viscosity is not None else options.horizontal_viscosity
    if nu is None:
        raise ValueError('sediment_model_options.morphological_viscosity or horizontal_viscosity must be set: the sediment model '
                         'derives dstar and the settling velocity from it')
    vals = {name: _constant_value(name, getattr(so, name))
            for name in ('average_sediment_size', 'bed_reference_height', 'porosity', 'sediment_density')}
    nu = _constant_value('morphological_viscosity' if so.morphological_viscosity is not None else 'horizontal_viscosity (read by the '
                         'sediment model)', nu)
    return sediment_constants(vals['average_sediment_size'], vals['bed_reference_height'], nu, vals['sediment_density'],
                              rho0=float(physical_constants['rho0']), g=float(physical_constants['g_grav']),
                              kappa=float(physical_constants['von_karman']), porosity=vals['porosity'],
                              morfac=float(so.morphological_acceleration_factor))


class SedimentEquation2D(object):
    """Descriptor of the sediment equation (thetis/sediment_eq_2d.py): the tracer equation's advection and diffusion on the same
    stage kernels, the source from the sediment model, and the ``'equilibrium'`` boundary key."""

    def __init__(self, function_space, depth, options, sediment_model, conservative=False):
        self.label = 'sediment_2d'
        self.function_space = function_space
        self.mesh = function_space.mesh()
        self.depth, self.options, self.sediment_model = depth, options, sediment_model
        self.conservative = bool(conservative)

    @staticmethod
    def check_bnd_conditions(bnd_conditions):
        from .tracer_eq_2d import TracerEquation2D
        plain = {}
        for marker, funcs in (bnd_conditions or {}).items():
            if funcs is not None and 'equilibrium' in funcs and 'value' in funcs:
                raise ValueError('Cannot specify both equilibrium and value for sediment bcs.')     # sediment_eq_2d.py:49-50
            plain[marker] = {k: v for k, v in (funcs or {}).items() if k != 'equilibrium'}
        TracerEquation2D.check_bnd_conditions(plain)


class SedimentModel(object):
    """``SedimentModel(options, mesh2d, uv, elev, depth)`` with the reference's attribute and method names where they apply
    (sediment_model.py:58-211).  ``uv`` / ``elev``: the DG-P1 solution Functions; ``depth``: a ``DepthExpression``.  The terms
    are nodal arrays (N, 3) that ``update()`` refreshes from the current ``uv`` and ``elev`` - on the device when one is bound
    (``bind_device``: the planes stay there and are read back on demand), through :class:`HostSediment` otherwise."""

    def __init__(self, options, mesh2d, uv, elev, depth, comm=None, tidal_farms=False):
        self.options, self.mesh2d, self.uv, self.elev, self.depth = options, mesh2d, uv, elev, depth
        so = options.sediment_model_options
        self.solve_suspended_sediment = so.solve_suspended_sediment
        self.use_bedload = so.use_bedload
        self.use_sediment_slide = so.use_sediment_slide
        self.use_angle_correction = so.use_angle_correction
        self.use_slope_mag_correction = so.use_slope_mag_correction
        self.use_advective_velocity_correction = so.use_advective_velocity_correction
        self.use_secondary_current = so.use_secondary_current
        self.constants = check_sediment_options(options, mesh2d, comm, tidal_farms)
        if self.use_angle_correction:
            print_output('WARNING: Slope effect angle correction only applies to bedload transport which is not used in this simulation')
        if self.use_slope_mag_correction:
            print_output('WARNING: Slope effect magnitude correction only applies to bedload transport which is not used in this simulation')
        c = self.constants
        self.average_size, self.bed_reference_height, self.rhos = so.average_sediment_size, so.bed_reference_height, so.sediment_density
        self.g, self.rhow, self.R = c['g'], c['rho0'], c['R']
        self.a, self.dstar, self.thetacr, self.taucr, self.settling_velocity = c['a'], c['dstar'], c['thetacr'], c['taucr'], c['ws']
        self.conservative = bool(so.use_sediment_conservative_form)
        self.host = HostSediment(mesh2d.cells, mesh2d.vertex_xy, c, conservative=self.conservative,
                                 nonlinear=bool(getattr(depth, 'use_nonlinear_equations', options.use_nonlinear_equations)))
        self._device = None
        self._planes = None

    def device_parameters(self):
        return device_parameters(self.constants, self.conservative, self.options.sediment_model_options.solve_exner)

    def bind_device(self, device, tracer_id):
        """the sediment field is tracer ``tracer_id`` of ``device``: the passes run there and the planes are read back on demand
        (a device class without ``sediment_set`` is not bound: the terms come from ``HostSediment``)"""
        if hasattr(device, 'sediment_set'):
            device.sediment_set(tracer_id, self.device_parameters())
            self._device = device

    @property
    def on_device(self):
        return self._device is not None

    def _bathymetry(self):
        b = self.depth.bathymetry_2d
        return b.dat.data_ro if isinstance(b, Function) else np.asarray(b, dtype=np.float64)

    def update(self):
        """refresh the terms from the current ``uv`` and ``elev`` (once per time step: the coefficients are frozen over it)"""
        if self._device is not None:
            self._device.sediment_update()
            self._planes = None
            return
        self._planes = self.host.coefficients(self.uv.cell_node_values(), self.elev.cell_node_values(), self._bathymetry())

    def _terms(self):
        if self._planes is None:
            if self._device is None:
                self.update()
            else:
                self._planes = self._device.sediment_read()
        return self._planes

    def get_erosion_term(self):
        """(depth-integrated) erosion at the DG nodes"""
        return self._terms()[0]

    def get_deposition_coefficient(self):
        """coefficient C such that C/H*sediment is the deposition term of the sediment equation"""
        return self._terms()[1]

    def get_equilibrium_tracer(self):
        """(depth-averaged) equilibrium concentration at the DG nodes"""
        return self._terms()[2]

    @property
    def equilibrium_tracer(self):
        return self.get_equilibrium_tracer()

    def get_advective_velocity_correction_factor(self):
        return 1
