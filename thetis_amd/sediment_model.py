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
           'bedload_constants', 'bedload_closures', 'bedload_device_parameters', 'open_bedload_markers', 'slide_constants',
           'slide_device_parameters', 'EXNER_MIN_DEPTH']

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


def slide_constants(c, max_angle=32.0, length_scale=0.0, porosity=0.4, morfac=1.0):
    """``sediment_constants`` (or ``bedload_constants``) plus what the sediment slide reads (sediment_model.py:312-354): the tangent of
    the angle of repose ``max_angle`` (degrees), the length scale L, the porosity and the morphological factor of the cosine"""
    s = dict(c)
    s.update(tanphi=float(np.tan(float(max_angle)*np.pi/180)), slide_length_scale=float(length_scale), porosity=float(porosity),
             morfac=float(morfac))
    return s


def slide_device_parameters(s, solve_exner=True, min_depth=EXNER_MIN_DEPTH):
    """``slide_constants`` -> the fields of include/swe2d.h swe2d_slide_params"""
    return dict(tanphi=s['tanphi'], length_scale=s['slide_length_scale'], porosity=s['porosity'], morfac=s['morfac'], fac=s['fac'],
                min_depth=float(min_depth), solve_exner=int(bool(solve_exner)))


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

    def slide_contributions(self, alpha, bath):
        """(N, 3): what each cell adds at its three nodes to the slide term  int alpha grad(psi) . grad(b) dx  of the Exner update,
        from the cell-constant ``alpha`` (N,) and the vertex bathymetry: (A*alpha)*(grad psi_i . grad b), the unscaled gradient"""
        alpha = np.asarray(alpha, dtype=np.float64)
        bx, by = self.gradient(np.asarray(bath, dtype=np.float64)[self.cells])
        A, gx, gy = self.area, self.grad_x, self.grad_y
        return np.stack([(A*alpha)*(gx[:, i]*bx + gy[:, i]*by) for i in range(3)], axis=1)

    def slide(self, bath, dt, region=None, constants=None):
        """the sediment slide on the vertex bathymetry ``bath`` with the step ``dt``: ``(alpha, beta, contrib, flagged)`` - the
        cell-constant diffusion coefficient (N,), the slope angle in radians (N,), the (N, 3) contributions to the Exner update and the
        number of flagged cells (alpha > 0, or dt above the per-cell bound of the explicit update).  ``region``: (N,) per cell or
        None; ``constants``: ``slide_constants`` (default: this object's).  Operation by operation what swe_slide_kernel does
        (include/swe2d.h has the formulas); asin and cos are numpy's."""
        s = self.c if constants is None else constants
        tanphi, L, porosity, morfac = s['tanphi'], s['slide_length_scale'], s['porosity'], s['morfac']
        bx, by = self.gradient(np.asarray(bath, dtype=np.float64)[self.cells])
        r = 1.0 if region is None else np.asarray(region, dtype=np.float64).reshape(bx.shape)
        sx, sy = r*bx, r*by
        s2 = sx*sx + sy*sy
        nz = 1.0/np.sqrt(1.0 + s2)
        sinb = np.sqrt(1.0 - nz*nz)
        tanbeta = sinb/nz
        beta = np.arcsin(sinb)
        d = tanbeta - tanphi
        slides = d > 0.0
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            cs = np.where(slides, np.cos(beta*dt*morfac), 1.0)
            qaval = np.where(slides, ((1.0 - porosity)*0.5*(L*L)*d)/cs, 0.0)
            steep = sinb > 0.0
            alpha = np.where(steep, -(qaval*(nz*nz))/np.where(steep, sinb, 1.0), 0.0)
            contrib = self.slide_contributions(alpha, bath)
        return alpha, beta, contrib, int(self.slide_flags(alpha, dt).sum())

    def slide_flags(self, alpha, dt):
        """(N,) bool: the cells a slide pass with this ``alpha`` flags - alpha > 0 (anti-diffusion), or
        dt*|alpha|*3*max_i |grad psi_i|^2 > 1, a sufficient per-cell bound for the lumped forward-Euler diffusion"""
        alpha = np.asarray(alpha, dtype=np.float64)
        gx, gy = self.grad_x, self.grad_y
        gmax = np.zeros_like(alpha)
        for i in range(3):
            g2 = gx[:, i]*gx[:, i] + gy[:, i]*gy[:, i]
            gmax = np.where(g2 > gmax, g2, gmax)
        with np.errstate(invalid='ignore', over='ignore'):
            return (alpha > 0.0) | (((dt*np.abs(alpha))*3.0)*gmax > 1.0)

    def exner(self, E, D, S, eta, bath, dt, bedload=None, slide=None):
        """one bed update: the new vertex bathymetry (vertices whose depth would fall below the floor keep theirs).  ``bedload``:
        the (N, 3) contributions of ``bedload_contributions``, gathered separately and added to the numerator; ``E`` = None: no
        sediment field (bedload only).  ``slide``: the (N, 3) contributions of ``slide``, gathered separately and scaled by ``dt``
        alone: b + ((dt*fac)*(num + nb) + dt*ns)/den"""
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
        nb = np.zeros(self.n_vertices)
        if bedload is not None:
            np.add.at(nb, vert, np.asarray(bedload, dtype=np.float64)[k, i])
        if slide is not None:
            ns = np.zeros(self.n_vertices)
            np.add.at(ns, vert, np.asarray(slide, dtype=np.float64)[k, i])
            b = bath + (dtf*(num + nb) + dt*ns)/np.where(used, den, 1.0)
        elif bedload is not None:
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
    if so.use_sediment_slide and not so.solve_exner:
        raise NotImplementedError('sediment_model_options.use_sediment_slide without solve_exner is not implemented: the slide enters '
                                  'the bed update only, and this build refuses an option it would ignore')
    if so.use_bedload and not so.solve_exner:
        raise NotImplementedError('sediment_model_options.use_bedload without solve_exner is not implemented: the bedload transport '
                                  'enters the bed update only, and this build refuses an option it would ignore')
    if so.use_secondary_current and not so.use_bedload:
        raise NotImplementedError('sediment_model_options.use_secondary_current without use_bedload is not implemented: the secondary '
                                  'current corrects the bedload transport only')
    if so.solve_suspended_sediment and so.use_advective_velocity_correction:
        raise NotImplementedError('sediment_model_options.use_advective_velocity_correction=True is not implemented (the tracer '
                                  'kernels take a scalar velocity factor): set it False')
    if so.solve_exner and not so.solve_suspended_sediment and not so.use_bedload and not so.use_sediment_slide:
        raise NotImplementedError('sediment_model_options.solve_exner without solve_suspended_sediment, use_bedload and '
                                  'use_sediment_slide: the bed update has no source (set one of the three)')
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
    if so.use_sediment_slide:
        par = {name: _constant_value(name, getattr(so, name)) for name in ('max_angle', 'sed_slide_length_scale')}
        if not par['sed_slide_length_scale'] > 0.0:
            raise NotImplementedError('sediment_model_options.use_sediment_slide with sed_slide_length_scale = {:g} is not '
                                      'implemented: the slide term is proportional to its square, and this build refuses an option '
                                      'it would ignore (set the length scale to about the mesh size)'.format(par['sed_slide_length_scale']))
        if not 0.0 < par['max_angle'] < 90.0:
            raise ValueError('sediment_model_options.max_angle must lie between 0 and 90 degrees')
        _slide_region(so.slide_region, mesh2d)          # (refused by name here, when the equations are built)
        c = slide_constants(c, par['max_angle'], par['sed_slide_length_scale'], vals['porosity'],
                            float(so.morphological_acceleration_factor))
    return c


def _slide_region(region, mesh2d):
    """``slide_region`` as one number per cell: None (no region), a Constant / number, a DG0 Function, or a CG-P1 Function reduced to
    the mean of its three vertex values; anything else is refused by name"""
    if region is None:
        return None
    if isinstance(region, (int, float, np.floating, Constant)):
        try:
            value = float(region)
        except TypeError:
            value = None
        if value is not None:
            return None if mesh2d is None else np.full(int(np.asarray(mesh2d.cells).shape[0]), value)
    if isinstance(region, Function) and not region.function_space().vector:
        fs = region.function_space()
        if fs.family == 'DG' and fs.degree == 0:
            return np.array(region.dat.data_ro, dtype=np.float64).reshape(-1)
        if fs.family == 'CG' and fs.degree == 1:
            v = np.asarray(region.dat.data_ro, dtype=np.float64).reshape(-1)[np.asarray(fs.mesh().cells)]
            return ((v[:, 0] + v[:, 1]) + v[:, 2])/3.0
    raise NotImplementedError('sediment_model_options.slide_region must be None, a Constant, a DG0 Function or a CG-P1 Function on '
                              'the device path (the slide region is one number per cell)')


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
        self._slide = None                      # (alpha, beta) of the last slide pass, per cell
        self._slide_max = 0.0                   # host path: the largest beta of the last pass, radians
        self.host_flagged = 0                   # host path: cells the slide passes flagged
        self.bnd_functions = {}                 # the shallow-water boundary dict: which markers the bedload transport leaves through

    def device_parameters(self):
        return device_parameters(self.constants, self.conservative, self.options.sediment_model_options.solve_exner)

    # q_b in the launch of the coefficient pass (swe2d_bedload_params.fuse_with_sediment): measured faster than a launch of its own
    # (DESIGN.md 5h), the same bits; without a sediment field there is no coefficient pass and the switch does nothing
    fuse_bedload = True

    def bedload_device_parameters(self):
        return bedload_device_parameters(self.constants, self.options.sediment_model_options.solve_exner,
                                         fuse_with_sediment=self.fuse_bedload)

    def slide_device_parameters(self):
        return slide_device_parameters(self.constants, self.options.sediment_model_options.solve_exner)

    def slide_region(self):
        """the slide region as one number per cell, or None (``_slide_region``)"""
        return _slide_region(self.options.sediment_model_options.slide_region, self.mesh2d)

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
            if self.use_sediment_slide and not hasattr(device, 'slide_set'):
                raise NotImplementedError('sediment_model_options.use_sediment_slide: the device class has the sediment passes but not '
                                          'the slide pass')
            device.sediment_set(tracer_id, self.device_parameters())
            self._bind_bed_passes(device)
            self._device = device

    def _bind_bed_passes(self, device):
        if self.use_bedload:
            device.bedload_set(self.bedload_device_parameters(), self.open_markers())
        if self.use_sediment_slide:
            device.slide_set(self.slide_device_parameters(), self.slide_region())

    def bind_bedload_device(self, device):
        """a run without a sediment field: the bedload pass, the slide pass and the bed update run on ``device``"""
        self._bind_bed_passes(device)
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

    def update_slide(self, dt):
        """refresh the slide from the current bed (once per time step, after the bedload pass); returns the contributions to the
        Exner update on the host path, None on the device (which takes the handle's step)"""
        self._slide = None
        if self._device is not None:
            self._device.slide_update()
            return None
        alpha, beta, contrib, flagged = self.host.slide(self._bathymetry(), float(dt), self.slide_region())
        self._slide = (alpha, beta)
        self._slide_max = float(beta.max()) if beta.size else 0.0
        self.host_flagged += flagged
        return contrib

    def _slide_planes(self):
        if not self.use_sediment_slide:
            raise ValueError('sediment_model_options.use_sediment_slide is off')
        if self._slide is None:
            if self._device is None:
                raise ValueError('the slide has not been evaluated yet (assign_initial_conditions does)')
            alpha, beta, _ = self._device.slide_read()
            self._slide = (alpha, beta)
        return self._slide

    def _dg0(self, values, name):
        from .function import get_functionspace
        f = Function(get_functionspace(self.mesh2d, 'DG', 0), name=name)
        f.dat.data[...] = values
        return f

    def get_sediment_slide_term(self, bathymetry=None):
        """the cell-constant diffusion coefficient alpha of the last slide pass as a DG0 Function (the reference returns the tensor
        alpha*I as an expression of ``bathymetry``; the bed is explicit here and the term is that of the current one)"""
        return self._dg0(self._slide_planes()[0], 'sediment_slide_alpha')

    @property
    def betaangle(self):
        """the slope angle of the bed (radians) of the last slide pass, DG0: ``beta.interpolate(sediment_model.betaangle)``"""
        return self._dg0(self._slide_planes()[1], 'betaangle')

    def max_slope_angle(self):
        """the largest slope angle of the last slide pass in degrees: one double from the device, not collective"""
        if not self.use_sediment_slide:
            raise ValueError('sediment_model_options.use_sediment_slide is off')
        rad = self._device.slide_max_angle() if self._device is not None else self._slide_max
        return rad*180.0/np.pi

    def slide_flagged(self):
        """cells flagged by the slide passes so far: alpha > 0 (the reference's cosine went negative) or a step above the per-cell
        bound of the explicit update"""
        if not self.use_sediment_slide:
            raise ValueError('sediment_model_options.use_sediment_slide is off')
        return int(self._device.slide_flagged()) if self._device is not None else self.host_flagged

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
