"""Shared by tests/test_slide.py, tests/test_gpu_slide.py and tests/test_gpu_slide_example.py: the parameters of the reference's slide
test, beds of which roughly half the cells are steeper than the angle of repose, the ramp of the reference's
``test/sediment/test_sed_slide.py``, and a scalar transcription of the reference's slide term (thetis/sediment_model.py:312-354,
thetis/exner_eq.py:132-149) with ``math`` only, importing nothing from thetis_amd/sediment_model.py."""
import math

import numpy as np

from bedload_cases import cell_gradient
from sediment_cases import D50, KS, NU
from thetis_amd.mesh import RectangleMesh

MAX_ANGLE, LENGTH, POROSITY, MORFAC, DT = 22.0, 0.2, 0.4, 20.0, 0.1
TANPHI = math.tan(MAX_ANGLE*math.pi/180)
RAMP_ANGLE = math.degrees(math.atan(0.5))                   # 26.565 degrees: the slope 0.5 of the ramp


def slide_c(morfac=MORFAC, max_angle=MAX_ANGLE, length=LENGTH, porosity=POROSITY):
    """the constants of a HostSediment / a device with the slide of the reference's test"""
    from thetis_amd.sediment_model import sediment_constants, slide_constants
    return slide_constants(sediment_constants(D50, KS, NU, porosity=porosity, morfac=morfac), max_angle, length, porosity, morfac)


def steep_bed(mesh, seed=0, offset=1.0, quantile=0.5):
    """a smooth random bed scaled so that the slope of the ``quantile`` cell is the tangent of the angle of repose: roughly half the
    cells slide.  The depth ``offset`` keeps the bed under water at rest."""
    rng = np.random.default_rng(seed)
    x, y = mesh.vertex_xy.T
    lx, ly = np.ptp(x), np.ptp(y)
    b = np.zeros_like(x)
    for _ in range(4):
        kx, ky = rng.integers(1, 4, size=2)
        px, py = rng.uniform(0, 2*np.pi, size=2)
        b += rng.uniform(0.5, 1.0)*np.sin(kx*np.pi*x/lx + px)*np.cos(ky*np.pi*y/ly + py)
    gx, gy = cell_gradient(mesh, b[mesh.cells])
    b *= 1.001*TANPHI/np.quantile(np.sqrt(gx*gx + gy*gy), quantile)       # (the quantile is a cell's own slope: keep it off the threshold)
    return offset + b - b.min()


def ramp_mesh():
    return RectangleMesh(20, 10, 4.0, 2.0)


def ramp_bed(mesh):
    """z_init of the reference's test: 0 | 0.5 x - 1"""
    x = mesh.vertex_xy[:, 0]
    return np.where(x < 2.0, 0.0, 0.5*x - 1.0)


def hat_gradients(mesh):
    """the gradients of the three hat functions of every cell, (N, 3) each, from the vertex coordinates by Cramer's rule on unit nodal
    values (not the library's table)"""
    n = mesh.num_cells
    gx, gy = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(3):
        e = np.zeros((n, 3))
        e[:, i] = 1.0
        gx[:, i], gy[:, i] = cell_gradient(mesh, e)
    return gx, gy


def cell_areas(mesh):
    xy = mesh.vertex_xy[mesh.cells]
    x, y = xy[..., 0], xy[..., 1]
    return 0.5*np.abs((x[:, 1] - x[:, 0])*(y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0])*(y[:, 1] - y[:, 0]))


def ref_slide_alpha(dzdx, dzdy, dt, region=None, max_angle=MAX_ANGLE, L=LENGTH, porosity=POROSITY, morfac=MORFAC):
    """get_sediment_slide_term at one point in plain Python floats, line by line: (alphaconst, betaangle)"""
    tanphi = math.tan(max_angle*math.pi/180)
    if region is not None:
        dzdx = region*dzdx
        dzdy = region*dzdy
    nz = 1/math.sqrt(1 + (dzdx**2 + dzdy**2))
    betaangle = math.asin(math.sqrt(1 - (nz**2)))
    tanbeta = math.sqrt(1 - (nz**2))/nz
    qaval = ((1 - porosity)*0.5*(L**2)*(tanbeta - tanphi)/(math.cos(betaangle*dt*morfac))) if tanbeta - tanphi > 0 else 0
    alphaconst = (-qaval*(nz**2)/math.sqrt(1 - (nz**2))) if math.sqrt(1 - (nz**2)) > 0 else 0
    return alphaconst, betaangle


def ref_slide(mesh, bath, dt, region=None, **kw):
    """(alpha (N,), beta (N,), contrib (N, 3)) cell by cell: the reference's alpha and the volume integral of ExnerSedimentSlideTerm,
    -f_i with f_i = A grad(psi_i) . (alpha grad(-b)), on a continuous bed (the facet integrals vanish)"""
    bx, by = cell_gradient(mesh, np.asarray(bath)[mesh.cells])
    hx, hy = hat_gradients(mesh)
    A = cell_areas(mesh)
    n = mesh.num_cells
    alpha, beta, contrib = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    for k in range(n):
        alpha[k], beta[k] = ref_slide_alpha(float(bx[k]), float(by[k]), dt, None if region is None else float(region[k]), **kw)
        for i in range(3):
            f = A[k]*(hx[k, i]*(alpha[k]*(-bx[k])) + hy[k, i]*(alpha[k]*(-by[k])))
            contrib[k, i] = -f
    return alpha, beta, contrib
