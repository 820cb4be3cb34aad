"""Shared by tests/test_sediment.py and tests/test_gpu_sediment.py: meshes, states that reach every branch of the closures, and
straight-line Python restatements of the reference's formulas (thetis/sediment_model.py:136-211) that import nothing from
thetis_amd/sediment_model.py."""
import math
import os

import numpy as np

from thetis_amd.mesh import Mesh2d, RectangleMesh

D50, KS, NU, RHOS, RHO0, G, KAPPA = 160e-6, 0.025, 1e-6, 2650.0, 1000.0, 9.81, 0.4


def ref_constants(d=D50, ks=KS, nu=NU, rhos=RHOS, rho0=RHO0, g=G):
    """dstar, thetacr, taucr, ws as the reference writes them"""
    R = rhos/rho0 - 1
    dstar = d*((g*R)/(nu**2))**(1/3)
    if dstar < 4:
        thetacr = 0.24*(dstar**(-1))
    elif dstar < 10:
        thetacr = 0.14*(dstar**(-0.64))
    elif dstar < 20:
        thetacr = 0.04*(dstar**(-0.1))
    elif dstar < 150:
        thetacr = 0.013*(dstar**(0.29))
    else:
        thetacr = 0.055
    taucr = (rhos - rho0)*g*d*thetacr
    if d <= 1e-04:
        ws = g*(d**2)*R/(18*nu)
    elif d <= 1e-03:
        ws = (10*nu/d)*(math.sqrt(1 + 0.01*((R*g*(d**3))/(nu**2))) - 1)
    else:
        ws = 1.1*math.sqrt(g*d*R)
    return dict(R=R, dstar=dstar, thetacr=thetacr, taucr=taucr, ws=ws)


def ref_closures(u, v, H, d=D50, ks=KS, nu=NU, rhos=RHOS, rho0=RHO0, g=G, kappa=KAPPA):
    """the reference's expressions at one point, in plain Python floats"""
    c = ref_constants(d, ks, nu, rhos, rho0, g)
    ws, taucr, dstar = c['ws'], c['taucr'], c['dstar']
    ksp, a = 3*d, ks/2
    hc = H if H > 0.001 else 0.001
    aux = 11.036*hc/ks if 11.036*hc/ks > 1.001 else 1.001
    qfc = 2/(math.log(aux)/kappa)**2
    cfactor = 2*(((1/kappa)*math.log(11.036*H/ksp))**(-2)) if H > ksp else 0.0
    mu = cfactor/qfc if qfc > 0 else 0.0
    unorm = u**2 + v**2
    B = 1.0 if a > H else a/H
    ustar = math.sqrt(0.5*qfc*unorm)
    rouse = ws/(kappa*ustar) - 1 if ustar > 0 else math.inf
    if abs(rouse) > 1e-04:
        step = B*(1 - B**min(rouse, 3))/min(rouse, 3)
    else:
        step = -B*math.log(B)
    integrated = max(1/step if step > 1e-12 else 1e12, 1)
    tau = rho0*0.5*qfc*unorm*mu
    T = (tau - taucr)/taucr if tau > 0 else -1
    cero = 0.015*(d/a)*(max(T, 0)**1.5)/(dstar**0.3)
    E, D = ws*cero, ws*integrated
    return dict(qfc=qfc, mu=mu, transport_stage_param=T, erosion_concentration=cero, rouse_number=rouse,
                integrated_rouse=integrated, erosion=E, deposition=D, equilibrium=E/D)


def union_jack(n=4, lx=4.0, ly=4.0):
    """n x n squares cut by alternating diagonals: interior vertices of valence 8 and 4"""
    xs, ys = np.linspace(0.0, lx, n + 1), np.linspace(0.0, ly, n + 1)
    xx, yy = np.meshgrid(xs, ys, indexing='ij')
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    vid = lambda i, j: i*(n + 1) + j
    cells = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            cells += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    mesh = Mesh2d(xy, np.array(cells), marker_fn=lambda xm, ym: np.where(np.abs(xm) < 1e-9, 1, 2))
    assert np.bincount(mesh.cells.ravel()).max() >= 8
    return mesh


def mesh_case(name):
    """'channel' 24 triangles of the 16 m x 1.1 m trench channel; 'coast' tests/golden/coast.msh (unstructured, as read); 'large'
    5000 triangles (20 workgroups of cells, a partial last wave of vertices); 'v63' / 'v64' / 'v65' 63, 64 and 65 vertices;
    'jack' a vertex of valence 8"""
    if name == 'channel':
        return RectangleMesh(6, 2, 16.0, 1.1)
    if name == 'small':                                 # the 4 x 3 mesh of the closed forms
        return RectangleMesh(4, 3, 16.0, 1.1)
    if name == 'large':
        return RectangleMesh(50, 50, 16.0, 1.1)
    if name in ('v63', 'v64', 'v65'):
        nx, ny = {'v63': (8, 6), 'v64': (7, 7), 'v65': (12, 4)}[name]
        mesh = RectangleMesh(nx, ny, 16.0, 1.1)
        assert mesh.vertex_xy.shape[0] == int(name[1:])
        return mesh
    if name == 'jack':
        return union_jack()
    from thetis_amd.meshio import read_gmsh
    return read_gmsh(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'coast.msh'))


def branch_state(mesh, seed=0, smooth=False):
    """(bath, uv, eta): nodal depths and speeds that reach, within one mesh, every branch of the closures: H below the grain
    roughness 3 d50 (and below the 0.001 floor of hc), H below the reference level a, ordinary depths; still water, speeds below and
    above the threshold of motion, Rouse numbers above 3, and nodes whose speed is built so that |rouse| <= 1e-4."""
    rng = np.random.default_rng(seed)
    n = mesh.num_cells
    x, y = mesh.vertex_xy.T
    bath = 1.0 + 0.2*np.sin(7.0*x/np.abs(x).max()) + 0.1*np.cos(5.0*y/np.abs(y).max())
    H = rng.uniform(0.2, 0.9, size=(n, 3))
    speed = rng.uniform(0.05, 1.4, size=(n, 3))
    if not smooth:
        kind = rng.integers(0, 12, size=(n, 3))
        H = np.where(kind == 0, rng.uniform(2e-4, 4e-4, size=(n, 3)), H)          # H <= ksp, hc = 0.001
        H = np.where(kind == 1, rng.uniform(2e-3, 1.0e-2, size=(n, 3)), H)         # a > H
        speed = np.where(kind == 2, 0.0, speed)                                    # still water
        speed = np.where(kind == 3, rng.uniform(0.01, 0.04, size=(n, 3)), speed)   # rouse > 3
        hc = np.where(H > 0.001, H, 0.001)
        ax = 11.036*hc/KS
        qfc = 2.0/(np.log(np.where(ax > 1.001, ax, 1.001))/KAPPA)**2
        ws = ref_constants()['ws']
        speed = np.where(kind == 4, (ws/KAPPA)/np.sqrt(0.5*qfc), speed)            # rouse = 0 to rounding
    ang = rng.uniform(0.0, 2*np.pi, size=(n, 3))
    uv = np.stack([speed*np.cos(ang), speed*np.sin(ang)], axis=2)
    eta = H - bath[mesh.cells]
    return bath, uv, eta


def threshold_margin(u, v, H):
    """smallest relative distance of a comparison operand of the closures to its threshold, per node (exact ties of structural
    zeros - still water - are no near misses: both sides compute the same zero)"""
    c = ref_constants()
    ws = c['ws']
    hc = np.where(H > 0.001, H, 0.001)
    ax = 11.036*hc/KS
    qfc = 2.0/(np.log(np.where(ax > 1.001, ax, 1.001))/KAPPA)**2
    deep = H > 3*D50
    lc = (1.0/KAPPA)*np.log(11.036*np.where(deep, H, 3*D50)/(3*D50))
    mu = np.where(deep, 2.0/(lc*lc), 0.0)/qfc
    unorm = u*u + v*v
    with np.errstate(divide='ignore', invalid='ignore'):
        rouse = ws/(KAPPA*np.sqrt(0.5*qfc*unorm)) - 1.0
        tau = RHO0*0.5*qfc*unorm*mu
        rel = lambda a, b: np.abs(a - b)/np.maximum(np.abs(b), 1e-300)
        m = np.minimum.reduce([rel(H, 0.001), rel(ax, 1.001), rel(H, 3*D50), rel(H, KS/2), rel(np.abs(rouse), 1e-4),
                               np.where(np.isfinite(rouse), rel(rouse, 3.0), 1.0),
                               np.where(tau > 0.0, rel(tau, c['taucr']), 1.0)])
    return m
