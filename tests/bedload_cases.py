"""Shared by tests/test_bedload.py and tests/test_gpu_bedload.py: states that reach both sides of the transport threshold with cells
at rest and sloping beds and surfaces, the distance of every new select to its threshold, and a scalar transcription of the
reference's bedload formulas (thetis/sediment_model.py:222-310) with ``math`` only, importing nothing from
thetis_amd/sediment_model.py."""
import itertools
import math

import numpy as np

from sediment_cases import D50, G, KAPPA, KS, NU, RHO0, RHOS, branch_state, ref_closures, ref_constants

BETA, SURBETA2, ALPHA_SECC = 1.3, 2/3, 0.75
SWITCHES = list(itertools.product((False, True), repeat=3))        # (magnitude, angle, secondary current)


def bedload_state(mesh, seed=0, smooth=False):
    """``branch_state`` with every seventh cell exactly at rest"""
    bath, uv, eta = branch_state(mesh, seed=seed, smooth=smooth)
    uv = uv.copy()
    uv[3::7] = 0.0
    return bath, uv, eta


def cell_gradient(mesh, nodal):
    """cell-constant gradient of nodal values (N, 3), by Cramer's rule on the vertex coordinates (not the library's table)"""
    xy = mesh.vertex_xy[mesh.cells]
    x, y = xy[..., 0], xy[..., 1]
    det = (x[:, 1] - x[:, 0])*(y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0])*(y[:, 1] - y[:, 0])
    f = np.asarray(nodal)
    gx = ((f[:, 1] - f[:, 0])*(y[:, 2] - y[:, 0]) - (f[:, 2] - f[:, 0])*(y[:, 1] - y[:, 0]))/det
    gy = ((x[:, 1] - x[:, 0])*(f[:, 2] - f[:, 0]) - (x[:, 2] - x[:, 0])*(f[:, 1] - f[:, 0]))/det
    return gx, gy


def ref_bedload(u, v, H, hx, hy, ex, ey, mag, ang, sec, beta=BETA, surbeta2=SURBETA2, alpha_secc=ALPHA_SECC):
    """the reference's expressions at one point in plain Python floats.  Where phi is zero the transport is (0, 0): the reference's
    u/sqrt(unorm) is 0/0 in water at rest, and this build defines the product as zero there."""
    c = ref_constants()
    cl = ref_closures(u, v, H)
    qfc, mu = cl['qfc'], cl['mu']
    R = RHOS/RHO0 - 1
    unorm = u**2 + v**2
    thetaprime = mu*(RHO0*0.5*qfc*unorm)/((RHOS - RHO0)*G*D50)
    phi = 0.0 if thetaprime < c['thetacr'] else 8*(thetaprime - c['thetacr'])**1.5
    if phi == 0.0:
        return 0.0, 0.0
    calfa, salfa = u/math.sqrt(unorm), v/math.sqrt(unorm)
    stress = RHO0*0.5*qfc*unorm
    slopecoef = 1 + beta*(hx*calfa + hy*salfa) if mag else 1.0
    if ang:
        cparam = (RHOS - RHO0)*G*D50*(surbeta2**2)
        tt1 = math.sqrt(cparam/stress) if stress > 1e-10 else math.sqrt(cparam/1e-10)
        aa = salfa + tt1*hy
        bb = calfa + tt1*hx
        comb = math.sqrt(aa**2 + bb**2)
        angle_norm = comb if comb > 1e-10 else 1e-10
        calfamod = (calfa + (tt1*hx))/angle_norm
        salfamod = (salfa + (tt1*hy))/angle_norm
    if sec:
        velocity_slide = (u*ey) - (v*ex)
        tandelta_factor = 7*G*RHO0*H*qfc/(2*alpha_secc*((u**2) + (v**2)))
        if ang:
            t_1 = (stress*slopecoef*calfamod) + (v*tandelta_factor*velocity_slide)
            t_2 = (stress*slopecoef*salfamod) - (u*tandelta_factor*velocity_slide)
        else:
            t_1 = (stress*slopecoef*calfa) + (v*tandelta_factor*velocity_slide)
            t_2 = ((stress*slopecoef*salfa) - (u*tandelta_factor*velocity_slide))
        t4 = math.sqrt((t_1**2) + (t_2**2))
        if t4 == 0.0:
            return 0.0, 0.0
        slopecoef_secc = t4/stress
        calfanew, salfanew = t_1/t4, t_2/t4
        qb_total = slopecoef_secc*phi*math.sqrt(G*R*D50**3)
        return qb_total*calfanew, qb_total*salfanew
    qb_total = slopecoef*phi*math.sqrt(G*R*D50**3)
    if ang:
        return qb_total*calfamod, qb_total*salfamod
    return qb_total*calfa, qb_total*salfa


def bedload_margin(u, v, H, hx, hy, ex, ey):
    """smallest relative distance of an operand of the bedload selects to its threshold, per node, with every correction on:
    thetaprime against thetacr, and at the moving nodes stress and the angle norm against 1e-10 and t4 against 0 (relative to the
    uncorrected stress).  Nodes at rest tie structurally: both sides compute the same zero."""
    c = ref_constants()
    hc = np.where(H > 0.001, H, 0.001)
    ax = 11.036*hc/KS
    qfc = 2.0/(np.log(np.where(ax > 1.001, ax, 1.001))/KAPPA)**2
    deep = H > 3*D50
    lc = (1.0/KAPPA)*np.log(11.036*np.where(deep, H, 3*D50)/(3*D50))
    mu = np.where(deep, 2.0/(lc*lc), 0.0)/qfc
    unorm = u*u + v*v
    stress = RHO0*0.5*qfc*unorm
    theta = mu*stress/((RHOS - RHO0)*G*D50)
    moves = theta > c['thetacr']
    rel = lambda a, b: np.abs(a - b)/np.maximum(np.abs(b), 1e-300)
    m = np.where(unorm > 0, rel(theta, c['thetacr']), 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        sn = np.where(moves, np.sqrt(unorm), 1.0)
        ca, sa = u/sn, v/sn
        tt1 = np.sqrt((RHOS - RHO0)*G*D50*SURBETA2**2/np.maximum(stress, 1e-10))
        aa, bb = sa + tt1*hy, ca + tt1*hx
        comb = np.sqrt(aa*aa + bb*bb)
        slope = 1.0 + BETA*(hx*ca + hy*sa)
        tdf = 7.0*G*RHO0*H*qfc/(2.0*ALPHA_SECC*np.where(moves, unorm, 1.0))
        vs = u*ey - v*ex
        t1 = stress*slope*bb/np.maximum(comb, 1e-10) + v*tdf*vs
        t2 = stress*slope*aa/np.maximum(comb, 1e-10) - u*tdf*vs
        t4 = np.sqrt(t1*t1 + t2*t2)
        at_moving = np.minimum.reduce([rel(stress, 1e-10), rel(comb, 1e-10), t4/np.where(moves, stress, 1.0)])
    return np.minimum(m, np.where(moves, at_moving, 1.0))
