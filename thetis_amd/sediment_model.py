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
           'bedload_constants', 'bedload_closures', 'bedload_device_parameters', 'open_bedload_markers', 'EXNER_MIN_DEPTH']

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
    c = dict(average_size=d, R=R, rhos=rhos, dstar=dstar, thetacr=thetacr, taucr=(rhos - rho0)*g*d*thetacr,
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
        unorm, qfc, cfactor, mu = _friction(c, u, v, H)
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


def _friction(c, u, v, H):
    """unorm, qfc, cfactor, mu: the lines of ``closures`` that the bedload shares (swe_sediment_friction on the device)"""
    kappa, ks, ksp = c['kappa'], c['ks'], c['ksp']
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
    return unorm, qfc, cfactor, mu


def bedload_constants(c, slope_effect_parameter=1.3, slope_effect_angle_parameter=2/3, secondary_current_parameter=0.75,
                      use_slope_mag_correction=True, use_angle_correction=True, use_secondary_current=False):
    """``sediment_constants`` plus what the bedload closures read (sediment_model.py:104-119, 222-310)"""
    d, g = c['average_size'], c['g']
    b = dict(c)
    b.update(beta=float(slope_effect_parameter), surbeta2=float(slope_effect_angle_parameter),
             alpha_secc=float(secondary_current_parameter), shields_den=(c['rhos'] - c['rho0'])*g*d,
             qb_scale=float(np.sqrt(g*c['R']*d**3)), use_slope_mag_correction=bool(use_slope_mag_correction),
             use_angle_correction=bool(use_angle_correction), use_secondary_current=bool(use_secondary_current))
    return b


def bedload_closures(b, u, v, H, hx, hy, ex, ey):
    """Meyer-Peter-Mueller transport (qbx, qby) with the slope and secondary current corrections at points with velocity (u, v),
    total depth H, bed gradient (hx, hy) and free-surface gradient (ex, ey): arrays that broadcast to one shape.  Operation by
    operation what swe_bedload_node does on the device (include/swe2d.h has the formulas); every conditional is a select, and a
    divisor that can vanish where nothing moves is replaced by 1 there."""
    u, v, H, hx, hy, ex, ey = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (u, v, H, hx, hy, ex, ey)))
    unorm, qfc, _, mu = _friction(b, u, v, H)
    stress = b['rho0']*0.5*qfc*unorm
    thetaprime = mu*stress/b['shields_den']
    moves = thetaprime > b['thetacr']
    x = np.where(moves, thetaprime - b['thetacr'], 0.0)
    phi = np.where(moves, 8.0*x*np.sqrt(x), 0.0)
    sn = np.where(moves, np.sqrt(unorm), 1.0)
    calfa, salfa = u/sn, v/sn
    slopecoef = 1.0 + b['beta']*(hx*calfa + hy*salfa) if b['use_slope_mag_correction'] else np.ones_like(u)
    ca, sa = calfa, salfa
    if b['use_angle_correction']:
        cparam = b['shields_den']*(b['surbeta2']*b['surbeta2'])
        tt1 = np.sqrt(cparam/np.where(stress > 1e-10, stress, 1e-10))
        aa, bb = salfa + tt1*hy, calfa + tt1*hx
        comb = np.sqrt(aa*aa + bb*bb)
        nrm = np.where(comb > 1e-10, comb, 1e-10)
        ca, sa = bb/nrm, aa/nrm
    factor, live = slopecoef, phi > 0.0
    if b['use_secondary_current']:
        vs = u*ey - v*ex
        tdf = 7.0*b['g']*b['rho0']*H*qfc/(2.0*b['alpha_secc']*np.where(moves, unorm, 1.0))
        t1 = stress*slopecoef*ca + v*tdf*vs
        t2 = stress*slopecoef*sa - u*tdf*vs
        t4 = np.sqrt(t1*t1 + t2*t2)
        t4s = np.where(t4 > 0.0, t4, 1.0)
        factor = t4/np.where(moves, stress, 1.0)
        ca, sa = t1/t4s, t2/t4s
        live = live & (t4 > 0.0)
    qtot = factor*phi*b['qb_scale']
    return np.where(live, qtot*ca, 0.0), np.where(live, qtot*sa, 0.0)


def bedload_device_parameters(b, solve_exner=True, min_depth=EXNER_MIN_DEPTH, fuse_with_sediment=False):
    """``bedload_constants`` -> the fields of include/swe2d.h swe2d_bedload_params but ``open_markers`` (Swe2dDevice.bedload_set
    builds the mask from a list of markers)"""
    p = {k: b[k] for k in ('beta', 'surbeta2', 'alpha_secc', 'thetacr', 'shields_den', 'qb_scale', 'ks', 'ksp', 'kappa', 'rho0', 'fac')}
    p.update(min_depth=float(min_depth), solve_exner=int(bool(solve_exner)), fuse_with_sediment=int(bool(fuse_with_sediment)),
             **{k: int(b[k]) for k in ('use_slope_mag_correction', 'use_angle_correction', 'use_secondary_current')})
    return p


def _is_zero(v):
    """``float(v) == 0.0`` of the reference's rule; a Function, a tidal forcing or anything without a float() counts as non-zero"""
    try:
        return float(v) == 0.0
    except (TypeError, ValueError):
        return False


def open_bedload_markers(bnd_functions, markers=None):
    """The markers open to the bedload transport by the reference's rule (exner_eq.py:113-125) on the shallow-water boundary dict:
    a marker absent from the dict is closed; so is one with a key other than 'elev' / 'uv' whose value is zero, or with a 'uv' whose
    components are all zero; every other marker is open.  ``markers``: restrict to these."""
    out = []
    for marker, funcs in (bnd_functions or {}).items():
        if funcs is None or (markers is not None and marker not in markers):
            continue
        closed = False
        for key, val in funcs.items():
            if key not in ('elev', 'uv'):
                closed = closed or _is_zero(val)
            elif key == 'uv':
                try:
                    comps = None if isinstance(val, Function) else list(val)
                except TypeError:
                    comps = None                                         # not a sequence of numbers: non-zero
                if comps is not None and all(_is_zero(j) for j in comps):
                    closed = True
        if not closed:
            out.append(marker)
    return out


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
        # the gradients of the three hat functions, (N, 3) each, formed as the library's host part forms them (include/swe2d.h)
        with np.errstate(divide='ignore', invalid='ignore'):
            det = p - q
            self.grad_x = np.stack([(y[:, 1] - y[:, 2])/det, (y[:, 2] - y[:, 0])/det, (y[:, 0] - y[:, 1])/det], axis=1)
            self.grad_y = np.stack([(x[:, 2] - x[:, 1])/det, (x[:, 0] - x[:, 2])/det, (x[:, 1] - x[:, 0])/det], axis=1)
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

    def gradient(self, nodal):
        """cell-constant gradient of the P1 interpolant of (N, 3) nodal values: (gx, gy), each (N,)"""
        f, gx, gy = np.asarray(nodal, dtype=np.float64), self.grad_x, self.grad_y
        return ((f[:, 0]*gx[:, 0] + f[:, 1]*gx[:, 1]) + f[:, 2]*gx[:, 2],
                (f[:, 0]*gy[:, 0] + f[:, 1]*gy[:, 1]) + f[:, 2]*gy[:, 2])

    def bedload(self, uv, eta, bath, constants=None):
        """nodal bedload transport (N, 3, 2) from nodal ``uv`` (N, 3, 2), ``eta`` (N, 3) and the vertex bathymetry; ``constants``:
        ``bedload_constants`` (default: this object's constants, which then must hold them)"""
        b = self.c if constants is None else constants
        uv, eta = np.asarray(uv, dtype=np.float64), np.asarray(eta, dtype=np.float64)
        hx, hy = self.gradient(np.asarray(bath, dtype=np.float64)[self.cells])
        ex, ey = self.gradient(eta) if self.nonlinear else (np.zeros_like(hx), np.zeros_like(hy))
        qx, qy = bedload_closures(b, uv[..., 0], uv[..., 1], self.depth(eta, bath), hx[:, None], hy[:, None], ex[:, None], ey[:, None])
        return np.stack([qx, qy], axis=2)

    def bedload_contributions(self, qb, cell_nbr=None, open_markers=0):
        """(N, 3): what each cell adds at its three nodes to the integral of div q_b against the vertex hat functions, the boundary
        integral over the open facets included.  ``cell_nbr``: (N, 3) facet codes (facet f joins the nodes f and (f+1)%3; a boundary
        facet carries minus its marker); ``open_markers``: bit m set = marker m is open, or an iterable of markers."""
        qb = np.asarray(qb, dtype=np.float64)
        qx, qy, A, gx, gy = qb[..., 0], qb[..., 1], self.area, self.grad_x, self.grad_y
        if not isinstance(open_markers, (int, np.integer)):
            open_markers = sum(1 << int(m) for m in set(open_markers))
        mx = ((qx[:, 0] + qx[:, 1]) + qx[:, 2])/3.0
        my = ((qy[:, 0] + qy[:, 1]) + qy[:, 2])/3.0
        c = [-(A*(mx*gx[:, i] + my*gy[:, i])) for i in range(3)]
        if cell_nbr is not None and open_markers:
            nbr = np.asarray(cell_nbr, dtype=np.int64)
            for f in range(3):
                b, o = (f + 1) % 3, (f + 2) % 3
                slot = np.where(nbr[:, f] < 0, -nbr[:, f], 0)
                is_open = (nbr[:, f] < 0) & (slot < 32) & (((int(open_markers) >> np.minimum(slot, 31)) & 1) == 1)
                Nx, Ny = -((2.0*A)*gx[:, o]), -((2.0*A)*gy[:, o])
                ta = ((2.0*qx[:, f] + qx[:, b])*Nx + (2.0*qy[:, f] + qy[:, b])*Ny)/6.0
                tb = ((2.0*qx[:, b] + qx[:, f])*Nx + (2.0*qy[:, b] + qy[:, f])*Ny)/6.0
                c[f] = np.where(is_open, c[f] + ta, c[f])
                c[b] = np.where(is_open, c[b] + tb, c[b])
        return np.stack(c, axis=1)

    def exner(self, E, D, S, eta, bath, dt, bedload=None):
        """one bed update: the new vertex bathymetry (vertices whose depth would fall below the floor keep theirs).  ``bedload``:
        the (N, 3) contributions of ``bedload_contributions``, gathered separately and added to the numerator; ``E`` = None: no
        sediment field (bedload only)"""
        bath = np.asarray(bath, dtype=np.float64)
        r = self.net_erosion(E, D, S, eta, bath) if E is not None else np.zeros(self.cells.shape)
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
        if bedload is not None:
            nb = np.zeros(self.n_vertices)
            np.add.at(nb, vert, np.asarray(bedload, dtype=np.float64)[k, i])
            b = bath + (dtf*(num + nb))/np.where(used, den, 1.0)
        else:
            b = bath + (dtf*num)/np.where(used, den, 1.0)
        ok = used & ((eta_min + b if self.nonlinear else b) >= self.min_depth)
        self.n_skipped += int((used & ~ok).sum())
        new = np.where(ok, b, bath)
        return new


def _constant_value(name, v):
    """a Constant / number of the sediment options; Functions and expressions are not on this path"""
    if isinstance(v, (int, float, np.floating, Constant)):
        try:
            return float(v)
        except TypeError:                       # (a vector Constant: what the options make of an array)
            pass
    raise NotImplementedError('sediment_model_options.{:} must be a Constant on the device path (a spatially varying value '
                              'is not implemented)'.format(name))


def check_sediment_options(options, mesh2d=None, comm=None, tidal_farms=False):
    """What this build refuses of the sediment options, each by the option's name; returns the run's constants
    (``sediment_constants``).  Called when the equations are built."""
    from .shallowwater_eq import physical_constants
    so = options.sediment_model_options
    if so.use_sediment_slide:
        raise NotImplementedError('sediment_model_options.use_sediment_slide is not implemented: this build runs the suspended load '
                                  'and the bedload transport (the slide is a diffusion of the bed of its own)')
    if so.use_bedload and not so.solve_exner:
        raise NotImplementedError('sediment_model_options.use_bedload without solve_exner is not implemented: the bedload transport '
                                  'enters the bed update only, and this build refuses an option it would ignore')
    if so.use_secondary_current and not so.use_bedload:
        raise NotImplementedError('sediment_model_options.use_secondary_current without use_bedload is not implemented: the secondary '
                                  'current corrects the bedload transport only')
    if so.solve_suspended_sediment and so.use_advective_velocity_correction:
        raise NotImplementedError('sediment_model_options.use_advective_velocity_correction=True is not implemented (the tracer '
                                  'kernels take a scalar velocity factor): set it False')
    if so.solve_exner and not so.solve_suspended_sediment and not so.use_bedload:
        raise NotImplementedError('sediment_model_options.solve_exner without solve_suspended_sediment and without use_bedload: the '
                                  'bed update has no source (set one of the two)')
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
    c = sediment_constants(vals['average_sediment_size'], vals['bed_reference_height'], nu, vals['sediment_density'],
                           rho0=float(physical_constants['rho0']), g=float(physical_constants['g_grav']),
                           kappa=float(physical_constants['von_karman']), porosity=vals['porosity'],
                           morfac=float(so.morphological_acceleration_factor))
    if so.use_bedload:
        par = {name: _constant_value(name, getattr(so, name))
               for name in ('slope_effect_parameter', 'slope_effect_angle_parameter', 'secondary_current_parameter')}
        c = bedload_constants(c, par['slope_effect_parameter'], par['slope_effect_angle_parameter'], par['secondary_current_parameter'],
                              so.use_slope_mag_correction, so.use_angle_correction, so.use_secondary_current)
    return c


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
        if self.use_angle_correction and not self.use_bedload:
            print_output('WARNING: Slope effect angle correction only applies to bedload transport which is not used in this simulation')
        if self.use_slope_mag_correction and not self.use_bedload:
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
        self._qb = None
        self.bnd_functions = {}                 # the shallow-water boundary dict: which markers the bedload transport leaves through

    def device_parameters(self):
        return device_parameters(self.constants, self.conservative, self.options.sediment_model_options.solve_exner)

    # q_b in the launch of the coefficient pass (swe2d_bedload_params.fuse_with_sediment): measured faster than a launch of its own
    # (DESIGN.md 5h), the same bits; without a sediment field there is no coefficient pass and the switch does nothing
    fuse_bedload = True

    def bedload_device_parameters(self):
        return bedload_device_parameters(self.constants, self.options.sediment_model_options.solve_exner,
                                         fuse_with_sediment=self.fuse_bedload)

    def open_markers(self):
        """the mesh markers open to the bedload transport (``open_bedload_markers`` on the shallow-water boundary dict)"""
        return open_bedload_markers(self.bnd_functions, markers=list(self.mesh2d.boundary_markers))

    def bind_device(self, device, tracer_id):
        """the sediment field is tracer ``tracer_id`` of ``device``: the passes run there and the planes are read back on demand
        (a device class without ``sediment_set`` is not bound: the terms come from ``HostSediment``)"""
        if hasattr(device, 'sediment_set'):
            if self.use_bedload and not hasattr(device, 'bedload_set'):
                raise NotImplementedError('sediment_model_options.use_bedload: the device class has the sediment passes but not the '
                                          'bedload pass')
            device.sediment_set(tracer_id, self.device_parameters())
            if self.use_bedload:
                device.bedload_set(self.bedload_device_parameters(), self.open_markers())
            self._device = device

    def bind_bedload_device(self, device):
        """a run without a sediment field: the bedload pass and the bed update run on ``device``"""
        device.bedload_set(self.bedload_device_parameters(), self.open_markers())
        self._device = device

    @property
    def on_device(self):
        return self._device is not None

    def _bathymetry(self):
        b = self.depth.bathymetry_2d
        return b.dat.data_ro if isinstance(b, Function) else np.asarray(b, dtype=np.float64)

    def update(self):
        """refresh the terms from the current ``uv`` and ``elev`` (once per time step: the coefficients are frozen over it)"""
        self._qb = None
        if not self.solve_suspended_sediment:   # (bedload only: no coefficient planes)
            return
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

    def update_bedload(self):
        """refresh q_b from the current ``uv``, ``elev`` and bed (once per time step, after the sediment step and the limiter);
        returns the contributions to the Exner update on the host path, None on the device"""
        if self._device is not None:
            self._device.bedload_update()
            self._qb = None
            return None
        self._qb = self.host.bedload(self.uv.cell_node_values(), self.elev.cell_node_values(), self._bathymetry())
        slot = {m: i + 1 for i, m in enumerate(sorted(int(m) for m in self.mesh2d.boundary_markers))}
        nbr = np.asarray(self.mesh2d.cell_nbr, dtype=np.int64)
        lut = np.zeros(max(slot, default=0) + 1, dtype=np.int64)
        for m, s in slot.items():
            lut[m] = s
        nbr = np.where(nbr < 0, -lut[np.where(nbr < 0, -nbr, 0)], nbr)
        return self.host.bedload_contributions(self._qb, nbr, [slot[int(m)] for m in self.open_markers()])

    def get_bedload_term(self, bathymetry=None):
        """nodal bedload transport (qbx, qby), each (N, 3), of the last update (``bathymetry``: the reference's argument; the bed is
        explicit here and the transport is that of the current one)"""
        if not self.use_bedload:
            raise ValueError('sediment_model_options.use_bedload is off')
        if self._qb is None:
            if self._device is not None:
                qx, qy, _ = self._device.bedload_read()
                self._qb = np.stack([qx, qy], axis=2)
            else:
                self.update_bedload()
        return self._qb[..., 0], self._qb[..., 1]

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
