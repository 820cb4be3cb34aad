#!/usr/bin/env python
"""Exactly integrated weak forms: rounding-free, quadrature-free reference values for the linear shallow-water and tracer stages.

Run by hand (``python tests/golden/make_exact_weakform_golden.py`` rewrites tests/golden/exact_weakforms*.json.gz byte for byte) and by
tests/test_exact_weakforms.py, which regenerates two cases and compares them with the committed files to the last bit.

Independent by construction: this file imports nothing of ``oracle/``, ``thetis_amd/`` or ``tests/helpers.py`` and uses no numpy.  It
builds its own meshes (vertex list, cell list, explicit (cell, facet) -> marker table), restates the forms of the reference from its
UFL text (file:line under thetis/ of the reference, cited at every term) and integrates every term in closed form:
  cells      monomials of the reference coordinates: int x^a z^b = a! b!/(a+b+2)! on the reference triangle (the barycentric
             monomial formula with lambda_1 = x, lambda_2 = z), 1/((a+1)(b+1)) on the reference square, times the constant det J
  facets     monomials of the arc parameter s in [0, 1]: int s^a = 1/(a+1), times the facet length
All numbers are ``fractions.Fraction``; where a facet length is irrational (the four facets at the off-centre vertex of ``tri8``) they
are elements of Q(sqrt(d_1), ..., sqrt(d_k)) (class ``Alg``: exact arithmetic on sums q_d sqrt(d), d squarefree).  g = 9 and h = 16
make sqrt(h/g) = 4/3 rational; inputs are integers (coordinates) or multiples of 1/64, dt is dyadic: every input is exact in float64.

What is polynomial, hence covered (use_nonlinear_equations=False, flat bathymetry, no Lax-Friedrichs velocity term):
  ExternalPressureGradientTerm shallowwater_eq.py:353-393, HUDivTerm :416-450, get_bnd_functions :232-272 (all seven kinds),
  CoriolisTerm :623-634, LinearDragTerm :734-740, AtmosphericPressureTerm :658-663, WindStressTerm :643-649 (divided by the constant
  rho_0 h), MomentumSourceTerm :805-811, ContinuitySourceTerm :825-831, HorizontalViscosityTerm :554-616 (SIPG; with flat bathymetry
  the grad-depth term :613-614 vanishes: grad(total_h) = 0), the mass term equation.py:99-105, the tracer terms tracer_eq_2d.py
  :147-193, :226-278, :281-298, :341-395, :439-445 with a velocity whose facet-averaged normal component keeps one sign along every
  facet (asserted: sign() and abs() are then constants per facet), and the SSPRK33 update in Shu-Osher form (rungekutta.py:326-347,
  :870-952) with alpha, beta = 1, 3/4, 1/4, 1/3, 2/3.  No forcing here depends on time, so the stage times c = 0, 1, 1/2 do not enter.
What is not polynomial and stays with the oracle tests: quadratic / Manning / Nikuradse drag, boundary drag, Lax-Friedrichs velocity
stabilisation, the nonlinear equations, variable bathymetry, wetting-drying, general (non-affine) quadrilaterals.  This pin covers
signs, '+'/'-' sides, boundary externals, the mass inverse, the Shu-Osher update and the exactness of the quadrature rules on
polynomial integrands; it does not cover Firedrake's quadrature of non-polynomial terms.

Output per case: the configuration as floats, the exact tendency dt M^-1 R and the state after one step (two on the 72-cell meshes)
as [hi, lo] pairs of float.hex() in gzip-compressed JSON (data only) (hi: the correctly rounded double, lo: the rounded remainder), and ``share``: the relative inf-norm
difference between the exact tendency and the exact tendency with the case's feature removed (or its sign flipped).  A case whose
share is below 1e-3 is refused: a match would be no evidence."""
import gzip
import json
import os
import sys
from fractions import Fraction as Fr
from math import factorial, gcd, isqrt

G, H, RHO0 = Fr(9), Fr(16), Fr(1000)          # sqrt(H/G) = 4/3
C_HG, C_GH = Fr(4, 3), Fr(3, 4)               # sqrt(h/g), sqrt(g/h)
MIN_SHARE = 1e-3
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------- exact numbers
class Alg(object):
    """sum of q_d*sqrt(d) over squarefree d, q_d rational"""
    __slots__ = ('t',)

    def __init__(self, t):
        self.t = {d: q for d, q in t.items() if q}

    def __bool__(self):
        return bool(self.t)

    def __add__(self, o):
        t = dict(self.t)
        for d, q in (o.t if isinstance(o, Alg) else {1: Fr(o)}).items():
            t[d] = t.get(d, 0) + q
        return Alg(t)
    __radd__ = __add__

    def __neg__(self):
        return Alg({d: -q for d, q in self.t.items()})

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Alg):
            o = Fr(o)
            return Alg({d: q*o for d, q in self.t.items()})
        t = {}
        for d1, q1 in self.t.items():
            for d2, q2 in o.t.items():
                c = gcd(d1, d2)                                  # sqrt(d1) sqrt(d2) = c sqrt((d1/c)(d2/c))
                d = (d1//c)*(d2//c)
                t[d] = t.get(d, 0) + q1*q2*c
        return Alg(t)
    __rmul__ = __mul__

    def __truediv__(self, o):
        return self*(1/Fr(o))


def inv_sqrt(n):
    """1/sqrt(n) for a positive integer n: a Fraction if n is a square, else sqrt(d)/(m d) with n = m^2 d"""
    n = int(n)
    r = isqrt(n)
    if r*r == n:
        return Fr(1, r)
    m, d, p = 1, n, 2
    while p*p <= d:
        while d % (p*p) == 0:
            d //= p*p
            m *= p
        p += 1
    return Alg({d: Fr(1, m*d)})


_BITS = 600


def as_fraction(x):
    """x as a Fraction: exact for a Fraction, to 2^-600 relative for an Alg (square roots by integer isqrt)"""
    if not isinstance(x, Alg):
        return Fr(x)
    return sum((q*Fr(isqrt(d << (2*_BITS)), 1 << _BITS) for d, q in x.t.items()), Fr(0))


def hilo(x):
    f = as_fraction(x)
    hi = float(f)                   # int/int true division: correctly rounded
    lo = float(f - Fr(hi))
    return [hi.hex(), lo.hex()]


# ---------------------------------------------------------------- polynomials
class Poly(object):
    """polynomial in nv variables, {exponent tuple: coefficient}"""
    __slots__ = ('t', 'nv')

    def __init__(self, t, nv):
        self.t = {e: c for e, c in t.items() if c}
        self.nv = nv

    @staticmethod
    def const(c, nv):
        return Poly({(0,)*nv: c}, nv)

    def _co(self, o):
        return o if isinstance(o, Poly) else Poly.const(o, self.nv)

    def __add__(self, o):
        t = dict(self.t)
        for e, c in self._co(o).t.items():
            t[e] = t.get(e, 0) + c
        return Poly(t, self.nv)
    __radd__ = __add__

    def __neg__(self):
        return Poly({e: -c for e, c in self.t.items()}, self.nv)

    def __sub__(self, o):
        return self + (-self._co(o))

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if not isinstance(o, Poly):
            return Poly({e: c*o for e, c in self.t.items()}, self.nv)
        t = {}
        for e1, c1 in self.t.items():
            for e2, c2 in o.t.items():
                e = tuple(a + b for a, b in zip(e1, e2))
                t[e] = t.get(e, 0) + c1*c2
        return Poly(t, self.nv)
    __rmul__ = __mul__

    def diff(self, i):
        t = {}
        for e, c in self.t.items():
            if e[i]:
                e2 = e[:i] + (e[i] - 1,) + e[i + 1:]
                t[e2] = t.get(e2, 0) + c*e[i]
        return Poly(t, self.nv)

    def on_line(self, a, b):
        """restriction of a 2-variable polynomial to the segment a + s (b - a): polynomial in s"""
        out = Poly({}, 1)
        xs = [Poly({(0,): Fr(a[i]), (1,): Fr(b[i] - a[i])}, 1) for i in range(2)]
        for e, c in self.t.items():
            term = Poly.const(c, 1)
            for i in range(2):
                for _ in range(e[i]):
                    term = term*xs[i]
            out = out + term
        return out


def int_line(p):
    return sum((c*Fr(1, e[0] + 1) for e, c in p.t.items()), Fr(0))


X, Z, ONE = Poly({(1, 0): Fr(1)}, 2), Poly({(0, 1): Fr(1)}, 2), Poly.const(Fr(1), 2)
BASIS = {3: [ONE - X - Z, X, Z], 4: [(ONE - X)*(ONE - Z), X*(ONE - Z), X*Z, (ONE - X)*Z]}
REFNODE = {3: [(0, 0), (1, 0), (0, 1)], 4: [(0, 0), (1, 0), (1, 1), (0, 1)]}


def int_ref(p, k):
    """integral over the reference triangle (k = 3) or the reference square (k = 4)"""
    if k == 3:
        return sum((c*Fr(factorial(e[0])*factorial(e[1]), factorial(e[0] + e[1] + 2)) for e, c in p.t.items()), Fr(0))
    return sum((c*Fr(1, (e[0] + 1)*(e[1] + 1)) for e, c in p.t.items()), Fr(0))


def solve_exact(M, b):
    """M^-1 b for a small rational matrix M (Gauss-Jordan in Fractions); b entries may be Alg"""
    n = len(M)
    A = [[Fr(v) for v in row] + [Fr(int(i == j)) for j in range(n)] for i, row in enumerate(M)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[piv] = A[piv], A[c]
        A[c] = [v/A[c][c] for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                A[r] = [v - A[r][c]*w for v, w in zip(A[r], A[c])]
    inv = [row[n:] for row in A]
    return [sum((b[j]*inv[i][j] for j in range(n)), Fr(0)) for i in range(n)]


# ---------------------------------------------------------------- meshes
class Mesh(object):
    def __init__(self, name, vertices, cells, marker_of):
        """marker_of(pa, pb) -> marker of the exterior facet pa -> pb"""
        self.name, self.v, self.cells = name, [tuple(p) for p in vertices], [tuple(c) for c in cells]
        self.k = k = len(cells[0])
        self.geo = []
        for c in self.cells:
            p = [self.v[i] for i in c]
            if k == 4:
                assert tuple(p[1][i] + p[3][i] - p[0][i] for i in range(2)) == p[2], 'parallelograms only'
            o = p[2] if k == 3 else p[3]
            J = [[Fr(p[1][0] - p[0][0]), Fr(o[0] - p[0][0])], [Fr(p[1][1] - p[0][1]), Fr(o[1] - p[0][1])]]
            det = J[0][0]*J[1][1] - J[0][1]*J[1][0]
            assert det > 0, 'cells must be counter-clockwise'
            Ji = [[J[1][1]/det, -J[0][1]/det], [-J[1][0]/det, J[0][0]/det]]
            # physical gradient of the basis: d/dX = dx/dX d/dx + dz/dX d/dz, (x, z) = J^-1 (X - p0)
            gphi = [[b.diff(0)*Ji[0][c] + b.diff(1)*Ji[1][c] for c in range(2)] for b in BASIS[k]]
            mass = [[det*int_ref(bi*bj, k) for bj in BASIS[k]] for bi in BASIS[k]]      # equation.py:105 inner(solution, test)*dx
            self.geo.append(dict(det=det, area=det/2 if k == 3 else det, Ji=Ji, gphi=gphi, mass=mass))
        seen, self.interior, self.exterior = {}, [], []
        for K, c in enumerate(self.cells):
            for f in range(k):
                key = tuple(sorted((c[f], c[(f + 1) % k])))
                if key in seen:
                    self.interior.append((seen.pop(key), (K, f)))
                else:
                    seen[key] = (K, f)
        self.facet_markers = []
        for K, f in sorted(seen.values()):
            pa, pb = self.v[self.cells[K][f]], self.v[self.cells[K][(f + 1) % k]]
            self.exterior.append((K, f, int(marker_of(pa, pb))))
            self.facet_markers.append([K, f, int(marker_of(pa, pb))])
        self.bnd_len = {}
        for K, f, m in self.exterior:
            il = self.facet(K, f)[1]
            assert isinstance(il, Fr), 'boundary facets must have rational length'
            self.bnd_len[m] = self.bnd_len.get(m, 0) + 1/il

    def facet(self, K, f):
        """(N, 1/length, length): N = outward normal times length of facet f of the counter-clockwise cell K"""
        pa, pb = self.v[self.cells[K][f]], self.v[self.cells[K][(f + 1) % self.k]]
        tx, ty = pb[0] - pa[0], pb[1] - pa[1]
        il = inv_sqrt(tx*tx + ty*ty)
        return (Fr(ty), Fr(-tx)), il, il*(tx*tx + ty*ty)

    def field(self, K, vertex_values):
        """the P1 / Q1 function of cell K with the given nodal values"""
        return sum((b*v for b, v in zip(BASIS[self.k], vertex_values)), Poly({}, 2))

    def grad(self, K, p):
        Ji = self.geo[K]['Ji']
        return [p.diff(0)*Ji[0][c] + p.diff(1)*Ji[1][c] for c in range(2)]

    def trace(self, K, f, p, reverse=False):
        a, b = REFNODE[self.k][f], REFNODE[self.k][(f + 1) % self.k]
        return p.on_line(b, a) if reverse else p.on_line(a, b)


def _rect_markers(x0, x1, y0, y1):
    def fn(pa, pb):
        if pa[0] == pb[0] == x0:
            return 1
        if pa[0] == pb[0] == x1:
            return 2
        if pa[1] == pb[1] == y0:
            return 3
        assert pa[1] == pb[1] == y1
        return 4
    return fn


def tri_mesh(name, xs, ys, moved=None, avoid=None):
    """grid of rectangles, each cut into two triangles; the diagonal avoids vertex ``avoid`` where given, else alternates"""
    ny = len(ys)
    vid = lambda i, j: i*ny + j
    verts = [(x, y) for x in xs for y in ys]
    if moved:
        verts[vid(*moved[0])] = moved[1]
    cells = []
    for i in range(len(xs) - 1):
        for j in range(ny - 1):
            v00, v10, v11, v01 = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            through_00 = (avoid not in (v00, v11)) if avoid is not None and avoid in (v00, v10, v11, v01) else (i + j) % 2 == 0
            cells += [(v00, v10, v11), (v00, v11, v01)] if through_00 else [(v00, v10, v01), (v10, v11, v01)]
    return Mesh(name, verts, cells, _rect_markers(xs[0], xs[-1], ys[0], ys[-1]))


def quad_mesh(name, widths, shears):
    """parallelograms: columns of the given widths, rows displaced by the given shear vectors (all of integer length)"""
    xs = [sum(widths[:i]) for i in range(len(widths) + 1)]
    ss = [(sum(s[0] for s in shears[:j]), sum(s[1] for s in shears[:j])) for j in range(len(shears) + 1)]
    ny = len(ss)
    vid = lambda i, j: i*ny + j
    verts = [(x + s[0], s[1]) for x in xs for s in ss]
    cells = [(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)) for i in range(len(widths)) for j in range(len(shears))]
    left = {verts[vid(0, j)] for j in range(ny)}
    right = {verts[vid(len(widths), j)] for j in range(ny)}

    def marker(pa, pb):
        if pa in left and pb in left:
            return 1
        if pa in right and pb in right:
            return 2
        if pa[1] == pb[1] == 0:
            return 3
        assert pa[1] == pb[1] == ss[-1][1]
        return 4
    return Mesh(name, verts, cells, marker)


def meshes():
    # tri8: the interior vertex (9, 12) moved to (13, 11): no mirror symmetry, four facets of irrational length at it
    return {'tri8': tri_mesh('tri8', [0, 9, 18], [0, 12, 24], moved=((1, 1), (13, 11)), avoid=4),
            'tri345': tri_mesh('tri345', [3*i for i in range(7)], [4*j for j in range(7)]),
            'quad4': quad_mesh('quad4', [5, 6], [(3, 4), (5, 12)]),
            'quad72': quad_mesh('quad72', [5, 6, 5, 6, 5, 6, 5, 6, 5], [(3, 4), (5, 12)]*4)}


# ---------------------------------------------------------------- deterministic data: multiples of 1/64
class Lcg(object):
    def __init__(self, seed):
        self.s = seed

    def draw(self, lo, hi):
        """a multiple of 1/64 in [lo, hi]"""
        self.s = (self.s*6364136223846793005 + 1442695040888963407) % (1 << 64)
        n = int((hi - lo)*64)
        return Fr(lo) + Fr((self.s >> 33) % (n + 1), 64)

    def vec(self, n, lo, hi):
        return [self.draw(lo, hi) for _ in range(n)]


def at_cells(mesh, vertex_values):
    return [[vertex_values[v] for v in c] for c in mesh.cells]


# ---------------------------------------------------------------- shallow water residual
def bnd_value(mesh, K, f, v, vec=False):
    """trace on facet f of cell K of a boundary value: a constant, or vertex values of a P1 Function"""
    if isinstance(v, list) and len(v) == len(mesh.v):
        if vec:
            return [mesh.trace(K, f, mesh.field(K, [v[i][c] for i in mesh.cells[K]])) for c in range(2)]
        return mesh.trace(K, f, mesh.field(K, [v[i] for i in mesh.cells[K]]))
    if vec:
        return [Poly.const(Fr(v[c]), 1) for c in range(2)]
    return Poly.const(Fr(v), 1)


def get_bnd_functions(mesh, K, f, funcs, marker, eta_in, uv_in, n):
    """shallowwater_eq.py:232-272 with total depth = bathymetry (utility.py:992-996, linear equations)"""
    def un_times_n(un):
        return [un*n[0], un*n[1]]
    val = lambda key, vec=False: bnd_value(mesh, K, f, funcs[key], vec)
    area = H*mesh.bnd_len[marker]
    if 'elev' in funcs and 'uv' in funcs:                 # :243-245
        return val('elev'), val('uv', True)
    if 'elev' in funcs and 'un' in funcs:                 # :246-248
        return val('elev'), un_times_n(val('un'))
    if 'elev' in funcs and 'flux' in funcs:               # :249-253
        return val('elev'), un_times_n(val('flux')*(1/area))
    if 'elev' in funcs:                                   # :254-256
        return val('elev'), uv_in
    if 'uv' in funcs:                                     # :257-259
        return eta_in, val('uv', True)
    if 'un' in funcs:                                     # :260-262
        return eta_in, un_times_n(val('un'))
    if 'flux' in funcs:                                   # :263-267
        return eta_in, un_times_n(val('flux')*(1/area))
    raise Exception('Unsupported bnd type')


def swe_residual(mesh, uv, eta, cfg):
    """R = -f: (R_uv[K][i][c], R_eta[K][i]) for uv[K][i][c], eta[K][i]"""
    k = mesh.k
    n_cells = len(mesh.cells)
    fu = [[[Fr(0), Fr(0)] for _ in range(k)] for _ in range(n_cells)]
    fe = [[Fr(0) for _ in range(k)] for _ in range(n_cells)]
    bnd = cfg.get('bnd', {})
    src = cfg.get('sources', {})
    visc = cfg.get('viscosity')
    rsign = cfg.get('riemann_sign', 1)                    # -1 only in the 'share' of the closed-wall case
    B = BASIS[k]

    def cell_fields(K):
        u = [mesh.field(K, [uv[K][i][c] for i in range(k)]) for c in range(2)]
        return u, mesh.field(K, eta[K])

    def vfield(K, name):
        return mesh.field(K, [src[name][v] for v in mesh.cells[K]])

    def stress_of(nu, gu):
        """:564-569: nu*2*sym(grad(uv)) or nu*grad(uv); gu[c][j] = d u_c / d x_j"""
        if visc['grad_div']:
            return [[nu*(gu[c][j] + gu[j][c]) for j in range(2)] for c in range(2)]
        return [[nu*gu[c][j] for j in range(2)] for c in range(2)]

    def nu_field(K):
        nu = visc['nu']
        return mesh.field(K, [nu[v] for v in mesh.cells[K]]) if isinstance(nu, list) else Poly.const(Fr(nu), 2)

    # ---- dx
    for K in range(n_cells):
        geo = mesh.geo[K]
        det, gphi = geo['det'], geo['gphi']
        u, e = cell_fields(K)
        I = lambda p: det*int_ref(p, k)
        if visc:
            st = stress_of(nu_field(K), [mesh.grad(K, u[c]) for c in range(2)])
        for i in range(k):
            for c in range(2):
                fu[K][i][c] += I(-G*e*gphi[i][c])                                   # :361 -g*head*nabla_div(u_test)
                if 'coriolis' in src:                                               # :632-633
                    fu[K][i][c] += I(vfield(K, 'coriolis')*B[i]*(-u[1] if c == 0 else u[0]))
                if 'linear_drag' in src:                                            # :738
                    ld = src['linear_drag']
                    ld = vfield(K, 'linear_drag') if isinstance(ld, list) else Fr(ld)
                    fu[K][i][c] += I(u[c]*B[i]*ld)
                if 'atmospheric_pressure' in src:                                   # :662, residual -f
                    fu[K][i][c] += I(mesh.grad(K, vfield(K, 'atmospheric_pressure'))[c]*B[i])/RHO0
                if 'wind_stress' in src:                                            # :648, residual +f
                    fu[K][i][c] -= I(mesh.field(K, [src['wind_stress'][v][c] for v in mesh.cells[K]])*B[i])/(H*RHO0)
                if 'momentum_source' in src:                                        # :810, residual +f
                    fu[K][i][c] -= I(mesh.field(K, [src['momentum_source'][v][c] for v in mesh.cells[K]])*B[i])
                if visc:                                                            # :571 inner(grad(u_test), stress)
                    fu[K][i][c] += I(gphi[i][0]*st[c][0] + gphi[i][1]*st[c][1])
            fe[K][i] += I(-(gphi[i][0]*u[0] + gphi[i][1]*u[1])*H)                    # :422 -inner(grad(eta_test), total_h*uv)
            if 'volume_source' in src:                                              # :830, residual +f
                fe[K][i] -= I(vfield(K, 'volume_source')*B[i])

    # ---- dS
    cp = 3 if k == 3 else 4                                                         # :576 (p+1)(p+2)/2 | (p+1)^2, p = 1
    for (Kp, fp), (Km, fm) in mesh.interior:
        N, il, ln = mesh.facet(Kp, fp)
        n_p = [N[0]*il, N[1]*il]
        sides = []
        for K, f, rev, sg in ((Kp, fp, False, 1), (Km, fm, True, -1)):
            u, e = cell_fields(K)
            tr = lambda p, K=K, f=f, rev=rev: mesh.trace(K, f, p, rev)
            s = dict(K=K, n=[sg*n_p[0], sg*n_p[1]], u=[tr(u[0]), tr(u[1])], e=tr(e), phi=[tr(b) for b in B],
                     gphi=[[tr(g) for g in gp] for gp in mesh.geo[K]['gphi']])
            if visc:
                s['nu'] = tr(nu_field(K))
                s['stress'] = stress_of(s['nu'], [[tr(g) for g in mesh.grad(K, u[c])] for c in range(2)])
            sides.append(s)
        P, M = sides
        # :363 head_star = avg(head) + sqrt(avg(total_h)/g)*jump(uv, n);  jump(v, n) = v('+').n('+') + v('-').n('-')
        jump_un = sum(((P['u'][c] - M['u'][c])*n_p[c] for c in range(2)), Poly({}, 1))
        head_star = (P['e'] + M['e'])*Fr(1, 2) + jump_un*(C_HG*rsign)
        # :425-426 uv_rie = avg(uv) + sqrt(g/h)*jump(eta, n), hu_star = h*uv_rie
        hu_star = [((P['u'][c] + M['u'][c])*Fr(1, 2) + (P['e'] - M['e'])*(n_p[c]*C_GH*rsign))*H for c in range(2)]
        if visc:
            avg_nu = (P['nu'] + M['nu'])*Fr(1, 2)
            tj = [[(P['u'][c] - M['u'][c])*n_p[j] for j in range(2)] for c in range(2)]          # utility.py:818 tensor_jump(uv, n)
            if visc['grad_div']:
                sj = [[avg_nu*(tj[c][j] + tj[j][c]) for j in range(2)] for c in range(2)]        # :566
            else:
                sj = [[avg_nu*tj[c][j] for j in range(2)] for c in range(2)]                     # :569
            avg_st = [[(P['stress'][c][j] + M['stress'][c][j])*Fr(1, 2) for j in range(2)] for c in range(2)]
            # :577-582 sigma = sipg_factor*cp/(CellVolume/FacetArea), the larger of the two sides
            sigma = visc['sipg_factor']*cp*ln/min(mesh.geo[Kp]['area'], mesh.geo[Km]['area'])
        for S in sides:
            K, nn = S['K'], S['n']
            for i in range(k):
                ph = S['phi'][i]
                for c in range(2):
                    fu[K][i][c] += ln*int_line(head_star*ph)*(G*nn[c])                       # :366 g*head_star*jump(u_test, n)
                    if visc:
                        v = sum((sj[c][j]*ph*(sigma*nn[j])                                   # :584 sigma*inner(tensor_jump(u_test, n), stress_jump)
                                 - S['gphi'][i][j]*sj[c][j]*Fr(1, 2)                         # :585 -inner(avg(grad(u_test)), stress_jump)
                                 - avg_st[c][j]*ph*nn[j] for j in range(2)), Poly({}, 1))    # :586 -inner(tensor_jump(u_test, n), avg(stress))
                        fu[K][i][c] += ln*int_line(v)
                fe[K][i] += ln*int_line((hu_star[0]*nn[0] + hu_star[1]*nn[1])*ph)            # :427 inner(jump(eta_test, n), hu_star)

    # ---- ds
    for K, f, marker in mesh.exterior:
        N, il, ln = mesh.facet(K, f)
        n = [N[0]*il, N[1]*il]
        u, e = cell_fields(K)
        tr = lambda p: mesh.trace(K, f, p)
        gu = [[tr(g) for g in mesh.grad(K, u[c])] for c in range(2)]
        u, e = [tr(u[0]), tr(u[1])], tr(e)
        phi = [tr(b) for b in B]
        gphi = [[tr(g) for g in gp] for gp in mesh.geo[K]['gphi']]
        funcs = bnd.get(marker)
        vec = [Poly({}, 1), Poly({}, 1)]
        sca = Poly({}, 1)
        un = u[0]*n[0] + u[1]*n[1]
        if funcs:                                                                     # impose_dynamic_bnd :286-296
            eta_ext, uv_ext = get_bnd_functions(mesh, K, f, funcs, marker, e, u, n)
            un_jump = (u[0] - uv_ext[0])*n[0] + (u[1] - uv_ext[1])*n[1]               # :373
            eta_rie = (e + eta_ext)*Fr(1, 2) + un_jump*C_HG                          # :374
            vec = [eta_rie*(G*n[c]) for c in range(2)]                                # :375
            un_rie = ((u[0] + uv_ext[0])*n[0] + (u[1] + uv_ext[1])*n[1])*Fr(1, 2) + (e - eta_ext)*C_GH    # :438, h_av = h
            sca = un_rie*H                                                            # :441-442 h_rie = bathymetry (linear)
            if visc:
                delta = None
                if 'un' in funcs:                                                     # :594-595
                    d = un - bnd_value(mesh, K, f, funcs['un'])
                    delta = [d*n[0], d*n[1]]
                elif uv_ext is not u:                                                 # :597-600
                    delta = [u[0] - uv_ext[0], u[1] - uv_ext[1]]
                if delta is not None:
                    nu = tr(nu_field(K))
                    od = [[delta[c]*n[j] for j in range(2)] for c in range(2)]
                    if visc['grad_div']:
                        sj = [[nu*(od[c][j] + od[j][c]) for j in range(2)] for c in range(2)]      # :603
                    else:
                        sj = [[nu*od[c][j] for j in range(2)] for c in range(2)]                   # :605
                    st = stress_of(nu, gu)
                    sigma = visc['sipg_factor']*cp*ln/mesh.geo[K]['area']
                    for i in range(k):
                        for c in range(2):
                            v = sum((sj[c][j]*phi[i]*(sigma*n[j]) - gphi[i][j]*sj[c][j] - st[c][j]*phi[i]*n[j]
                                     for j in range(2)), Poly({}, 1))                               # :607-611
                            fu[K][i][c] += ln*int_line(v)
        else:
            head_rie = e + un*(C_HG*rsign)                                             # :379-380
            vec = [head_rie*(G*n[c]) for c in range(2)]                                # :381
        for i in range(k):
            for c in range(2):
                fu[K][i][c] += ln*int_line(vec[c]*phi[i])
            fe[K][i] += ln*int_line(sca*phi[i])
    return ([[[-v for v in node] for node in cell] for cell in fu], [[-v for v in cell] for cell in fe])


def swe_tendency(mesh, uv, eta, cfg):
    """dt M^-1 R (rungekutta.py:900-904)"""
    ru, re = swe_residual(mesh, uv, eta, cfg)
    dt = cfg['dt']
    ku, ke = [], []
    for K in range(len(mesh.cells)):
        M = mesh.geo[K]['mass']
        cols = [solve_exact(M, [ru[K][i][c]*dt for i in range(mesh.k)]) for c in range(2)]
        ku.append([[cols[0][i], cols[1][i]] for i in range(mesh.k)])
        ke.append(solve_exact(M, [re[K][i]*dt for i in range(mesh.k)]))
    return ku, ke


def _axpy(a, x, b, y, c, z):
    """a*x + b*y + c*z on nested lists"""
    if isinstance(x, list):
        return [_axpy(a, xi, b, yi, c, zi) for xi, yi, zi in zip(x, y, z)]
    return x*a + y*b + z*c


def ssprk33(tendency, state):
    """Shu-Osher form of SSPRK33 (rungekutta.py:326-347, :908-946): u1 = u0 + k(u0); u2 = 3/4 u0 + 1/4 u1 + 1/4 k(u1);
    u3 = 1/3 u0 + 2/3 u2 + 2/3 k(u2)"""
    u0 = state
    u1 = _axpy(Fr(1), u0, Fr(0), u0, Fr(1), tendency(u0))
    u2 = _axpy(Fr(3, 4), u0, Fr(1, 4), u1, Fr(1, 4), tendency(u1))
    return _axpy(Fr(1, 3), u0, Fr(2, 3), u2, Fr(2, 3), tendency(u2))


# ---------------------------------------------------------------- tracer residual
def tracer_residual(mesh, T, cfg):
    """R = -f of tracer_eq_2d.py: HorizontalAdvectionTerm :147-193 | ConservativeHorizontalAdvectionTerm :341-395, SourceTerm
    :293-298 | ConservativeSourceTerm :439-445, HorizontalDiffusionTerm :226-278.  tracer_advective_velocity_factor = 1."""
    k = mesh.k
    B = BASIS[k]
    tc = cfg['tracer']
    uvv = tc['uv']                                       # continuous P1 velocity, vertex values
    cons, lf, mu_c, tsrc = tc['conservative'], tc['lax_friedrichs'], tc.get('diffusivity'), tc.get('source')
    bnd = tc.get('bnd', {})
    sipg = tc.get('sipg_factor', 1)
    flip = tc.get('flip_upwind', False)                  # only in the 'share'
    ft = [[Fr(0) for _ in range(k)] for _ in mesh.cells]
    vel = lambda K: [mesh.field(K, [uvv[v][c] for v in mesh.cells[K]]) for c in range(2)]
    vf = lambda K, vals: mesh.field(K, [vals[v] for v in mesh.cells[K]])
    mu_of = lambda K: (vf(K, mu_c) if isinstance(mu_c, list) else Poly.const(Fr(mu_c), 2))
    cp = 3 if k == 3 else 4

    def one_sign(un_line, N_over_n):
        """sign of un_av along the facet; un_line is polynomial in s with un = N.u / len: the sign is that of its end values"""
        vals = [as_fraction(sum((c for e, c in un_line.t.items()), Fr(0))*N_over_n), as_fraction(un_line.t.get((0,), Fr(0))*N_over_n)]
        assert all(e[0] <= 1 for e in un_line.t), 'velocity must be P1 along the facet'
        assert vals[0]*vals[1] > 0, 'the normal velocity must keep one sign along every facet'
        return 1 if vals[0] > 0 else 0

    for K in range(len(mesh.cells)):
        geo = mesh.geo[K]
        I = lambda p: geo['det']*int_ref(p, k)
        u, c_ = vel(K), mesh.field(K, T[K])
        gc = mesh.grad(K, c_)
        for i in range(k):
            g = geo['gphi'][i]
            if cons:                                     # :355-356 -(Dx(test,0)*uv[0]*c + Dx(test,1)*uv[1]*c)
                ft[K][i] += I(-(g[0]*u[0] + g[1]*u[1])*c_)
            else:                                        # :159-160 -(Dx(uv[0]*test,0)*c + Dx(uv[1]*test,1)*c)
                ft[K][i] += I(-(mesh.grad(K, u[0]*B[i])[0] + mesh.grad(K, u[1]*B[i])[1])*c_)
            if tsrc is not None:                         # :297 / :443-444 (H = bathymetry, linear equations); residual +
                ft[K][i] -= I(vf(K, tsrc)*B[i])*(H if cons else 1)
            if mu_c is not None:                         # :238 inner(grad_test, diff_flux)
                ft[K][i] += I(mu_of(K)*(g[0]*gc[0] + g[1]*gc[1]))

    for (Kp, fp), (Km, fm) in mesh.interior:
        N, il, ln = mesh.facet(Kp, fp)
        n_p = [N[0]*il, N[1]*il]
        sides = []
        for K, f, rev, sg in ((Kp, fp, False, 1), (Km, fm, True, -1)):
            tr = lambda p, K=K, f=f, rev=rev: mesh.trace(K, f, p, rev)
            u, c_ = vel(K), mesh.field(K, T[K])
            s = dict(K=K, n=[sg*n_p[0], sg*n_p[1]], u=[tr(u[0]), tr(u[1])], c=tr(c_), phi=[tr(b) for b in B], sg=sg,
                     gphi=[[tr(g) for g in gp] for gp in mesh.geo[K]['gphi']], gc=[tr(g) for g in mesh.grad(K, c_)])
            if mu_c is not None:
                s['mu'] = tr(mu_of(K))
            sides.append(s)
        P, M = sides
        # :164-168 un_av = avg(uv).n('-'), s = (sign(un_av)+1)/2, c_up = c('-')*s + c('+')*(1-s)
        un_av = sum(((P['u'][c] + M['u'][c])*Fr(1, 2)*M['n'][c] for c in range(2)), Poly({}, 1))
        s_ = one_sign(un_av, ln)
        abs_un = un_av if s_ else -un_av                 # |un_av|: one sign along the facet
        if flip:
            s_ = 1 - s_
        c_up = M['c'] if s_ else P['c']
        flux_up = [(M if s_ else P)['c']*(M if s_ else P)['u'][c] for c in range(2)]           # :364
        if mu_c is not None:
            sigma = sipg*cp*ln/min(mesh.geo[Kp]['area'], mesh.geo[Km]['area'])                 # :243-249
            jump_c = [P['c']*P['n'][j] + M['c']*M['n'][j] for j in range(2)]                   # jump(c, n)
            avg_mu = (P['mu'] + M['mu'])*Fr(1, 2)
            avg_flux = [(P['mu']*P['gc'][j] + M['mu']*M['gc'][j])*Fr(1, 2) for j in range(2)]
        for S in sides:
            K, nn = S['K'], S['n']
            for i in range(k):
                ph = S['phi'][i]
                if cons:                                 # :366-367 flux_up[j]*jump(test, n[j])
                    v = (flux_up[0]*nn[0] + flux_up[1]*nn[1])*ph
                else:                                    # :170-171 c_up*(jump(test, uv[0]*n[0]) + jump(test, uv[1]*n[1]))
                    v = c_up*(S['u'][0]*nn[0] + S['u'][1]*nn[1])*ph
                if lf:                                   # :174-175 / :376-377 gamma*jump(test)*jump(c), gamma = |un_av|/2
                    v = v + abs_un*Fr(1, 2)*(ph*S['sg'])*(P['c'] - M['c'])
                if mu_c is not None:
                    jn = jump_c[0]*nn[0] + jump_c[1]*nn[1]
                    v = v + avg_mu*jn*ph*sigma                                                   # :251-253
                    v = v - S['mu']*(S['gphi'][i][0]*jump_c[0] + S['gphi'][i][1]*jump_c[1])*Fr(1, 2)   # :254-255
                    v = v - (avg_flux[0]*nn[0] + avg_flux[1]*nn[1])*ph                           # :256-257
                ft[K][i] += ln*int_line(v)

    for K, f, marker in mesh.exterior:
        N, il, ln = mesh.facet(K, f)
        n = [N[0]*il, N[1]*il]
        tr = lambda p: mesh.trace(K, f, p)
        u, c_ = vel(K), mesh.field(K, T[K])
        gc = [tr(g) for g in mesh.grad(K, c_)]
        u, c_in = [tr(u[0]), tr(u[1])], tr(c_)
        un = u[0]*n[0] + u[1]*n[1]
        funcs = bnd.get(marker)
        v = c_in*un                                       # :190-191 / :392-393 (closed: no funcs)
        vd = None
        if funcs is not None:
            # get_bnd_functions :94-115 with 'value' or 'diff_flux' only: uv_ext = uv_in, so uv_av = uv
            s_ = one_sign(un, ln)
            if flip:
                s_ = 1 - s_
            if 'value' in funcs:
                val = funcs['value']
                is_fn = isinstance(val, list)
                c_ext = tr(vf(K, val)) if is_fn else Poly.const(Fr(val), 1)
                g_ext = [tr(g) for g in mesh.grad(K, vf(K, val))] if is_fn else [Poly({}, 1)]*2
            else:
                c_ext, g_ext = c_in, gc
            v = (c_in if s_ else c_ext)*un                # :186-188 c_up*un_av  /  :388-390 flux_up.n (uv_ext = uv)
            if mu_c is not None:
                if 'diff_flux' in funcs:                  # :267-268
                    vd = Poly.const(-Fr(funcs['diff_flux']), 1)
                else:                                     # :270-276 -test*dot(mu*grad(c_up), n), grad(c_up) = s grad(c_in) + (1-s) grad(c_ext)
                    gup = gc if s_ else g_ext
                    vd = -tr(mu_of(K))*(gup[0]*n[0] + gup[1]*n[1])
        for i in range(k):
            ph = tr(B[i])
            ft[K][i] += ln*int_line(v*ph)
            if vd is not None:
                ft[K][i] += ln*int_line(vd*ph)
    return [[-v for v in cell] for cell in ft]


def tracer_tendency(mesh, T, cfg):
    r = tracer_residual(mesh, T, cfg)
    return [solve_exact(mesh.geo[K]['mass'], [v*cfg['dt'] for v in r[K]]) for K in range(len(mesh.cells))]


# ---------------------------------------------------------------- cases
def _flat(x):
    if isinstance(x, list):
        return [v for xi in x for v in _flat(xi)]
    return [x]


def _norm_diff(a, b):
    fa, fb = [float(as_fraction(v)) for v in _flat(a)], [float(as_fraction(v)) for v in _flat(b)]
    return max(abs(x - y) for x, y in zip(fa, fb))/max(abs(x) for x in fa)


def _floats(x):
    if isinstance(x, dict):
        return {str(k_): _floats(v) for k_, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_floats(v) for v in x]
    if isinstance(x, (bool, str)) or x is None:
        return x
    f = float(x)
    assert Fr(f) == Fr(x), 'inputs must be exact in float64'
    return f


def mesh_state(mesh, name):
    seed = {'tri8': 11, 'quad4': 12, 'tri345': 13, 'quad72': 14}[name]
    r = Lcg(seed)
    n, k = len(mesh.cells), mesh.k
    uv = [[[r.draw(-1, 1), r.draw(-1, 1)] for _ in range(k)] for _ in range(n)]
    eta = [[r.draw(-1, 1) for _ in range(k)] for _ in range(n)]
    T = [[r.draw(1, 3) for _ in range(k)] for _ in range(n)]
    return uv, eta, T


def case_table(mesh, name):
    """[(case name, group, cfg, cfg of the 'share')]; every coefficient field is a continuous P1 field given by vertex values"""
    r = Lcg(1000 + len(mesh.cells)*mesh.k)
    nv = len(mesh.v)
    dt = Fr(1, 16)
    fld = lambda lo, hi: r.vec(nv, lo, hi)
    vfld = lambda lo, hi: [[r.draw(lo, hi), r.draw(lo, hi)] for _ in range(nv)]
    flux = {m: Fr(int(mesh.bnd_len[m])*4) for m in mesh.bnd_len}         # flux/(h*len) = 1/4
    const = {'elev': Fr(3, 8), 'uv': [Fr(5, 16), Fr(-7, 32)], 'un': Fr(-9, 32)}
    field = {'elev': fld(-1, 1), 'uv': vfld(-1, 1), 'un': fld(-1, 1)}

    def funcs_of(keys, marker, fn=False):
        out = {}
        for key in keys:
            if key == 'flux':
                out[key] = [v*flux[marker]*2 for v in field['un']] if fn else flux[marker]
            else:
                out[key] = field[key] if fn else const[key]
        return out
    base = dict(dt=dt)
    cases = []
    if len(mesh.cells) <= 8:
        cases.append(('walls', 'walls', dict(base), dict(base, riemann_sign=-1)))
        kinds = [('elev',), ('uv',), ('un',), ('flux',), ('elev', 'uv'), ('elev', 'un'), ('elev', 'flux')]
        for j, keys in enumerate(kinds):
            m = 1 + j % 4
            cases.append(('bnd_' + '_'.join(keys), 'boundary', dict(base, bnd={m: funcs_of(keys, m)}), dict(base)))
        for j, keys in enumerate(kinds[:4]):
            m = 1 + (j + 2) % 4
            cases.append(('bnd_' + keys[0] + '_function', 'boundary', dict(base, bnd={m: funcs_of(keys, m, True)}), dict(base)))
    all4 = {1: funcs_of(('elev',), 1), 2: funcs_of(('un',), 2, True), 3: funcs_of(('elev', 'flux'), 3), 4: funcs_of(('uv',), 4)}
    srcs = dict(coriolis=fld(Fr(1, 4), 1), linear_drag=fld(Fr(1, 4), 1), atmospheric_pressure=fld(-2000, 2000),
                momentum_source=vfld(-1, 1), volume_source=fld(-1, 1), wind_stress=vfld(-8000, 8000))
    # the same four kinds with constant data: what the C restatement can express too
    all4_const = dict(all4)
    all4_const[2] = funcs_of(('un',), 2)
    if len(mesh.cells) <= 8:
        cases.append(('bnd_all_four', 'boundary', dict(base, bnd=all4), dict(base)))
        cases.append(('bnd_all_four_constant', 'boundary', dict(base, bnd=all4_const), dict(base)))
        for key in ('coriolis', 'linear_drag', 'atmospheric_pressure', 'momentum_source', 'volume_source', 'wind_stress'):
            cases.append(('src_' + key, 'source', dict(base, sources={key: srcs[key]}), dict(base)))
        cases.append(('src_linear_drag_constant', 'source', dict(base, sources={'linear_drag': Fr(3, 4)}), dict(base)))
        cases.append(('src_all', 'source', dict(base, sources=srcs), dict(base)))
        nu_p1 = fld(1, 2)
        bnd_v = {1: funcs_of(('uv',), 1), 2: funcs_of(('un',), 2), 3: funcs_of(('elev',), 3), 4: funcs_of(('elev', 'flux'), 4)}
        for nu, gd, sf in ((nu, gd, sf) for nu in (Fr(3, 2), nu_p1) for gd in (False, True) for sf in (1, 2)):
            nm = 'visc_{:}_graddiv{:d}_sipg{:d}'.format('p1' if isinstance(nu, list) else 'constant', gd, sf)
            cfg = dict(base, bnd=bnd_v, viscosity=dict(nu=nu, grad_div=gd, sipg_factor=sf))
            cases.append((nm, 'viscosity', cfg, dict(base, bnd=bnd_v)))
        # tracer: velocity (1, 3/8) + a small P1 perturbation: its normal component keeps one sign on every facet (asserted)
        tuv = [[1 + r.draw(Fr(-1, 32), Fr(1, 32)), Fr(3, 8) + r.draw(Fr(-1, 32), Fr(1, 32))] for _ in range(nv)]
        tb = {1: {'value': Fr(5, 2)}, 2: {'diff_flux': Fr(3, 16)}, 3: {'value': fld(1, 3)}}
        tsrc, mu_p1 = fld(-1, 1), fld(1, 2)
        for cons in (False, True):
            for lf in (False, True):
                nm = 'tracer_{:}{:}'.format('conservative' if cons else 'nonconservative', '_lf' if lf else '')
                tc = dict(uv=tuv, conservative=cons, lax_friedrichs=lf, source=tsrc, bnd=tb, sipg_factor=2 if lf else 1,
                          diffusivity=(mu_p1 if cons != lf else Fr(5, 4)))
                cases.append((nm, 'tracer', dict(base, tracer=tc), dict(base, tracer=dict(tc, flip_upwind=True))))
        # advection alone (no diffusion, constant 'value' boundaries): what the C tracer restatement can express
        for lf in (False, True):
            tc = dict(uv=tuv, conservative=False, lax_friedrichs=lf, source=tsrc, bnd={1: {'value': Fr(5, 2)}, 3: {'value': Fr(7, 4)}})
            cases.append(('tracer_advection' + ('_lf' if lf else ''), 'tracer', dict(base, tracer=tc),
                          dict(base, tracer=dict(tc, flip_upwind=True))))
    else:
        # constant boundary data and a constant drag: also within the C restatement (the case without sources keeps the Function)
        two = dict(coriolis=srcs['coriolis'], linear_drag=Fr(3, 4))
        cases.append(('all_four_coriolis_drag', 'combined', dict(base, bnd=all4_const, sources=two, steps=2), dict(base)))
        if mesh.k == 3:
            cases.append(('all_four', 'bare', dict(base, bnd=all4), dict(base)))
    return cases


def compute_case(mesh, name, cfg, alt, state):
    uv, eta, T = state
    out = dict(mesh=mesh.name, dt=cfg['dt'])
    for key in ('bnd', 'sources', 'viscosity', 'tracer'):
        if key in cfg:
            out[key] = cfg[key]
    out = _floats(out)
    if 'tracer' in cfg:
        k0 = tracer_tendency(mesh, T, cfg)
        k_alt = tracer_tendency(mesh, T, alt)
        step = ssprk33(lambda s: tracer_tendency(mesh, s, cfg), T)
        out['tendency'] = {'tracer': [hilo(v) for v in _flat(k0)]}
        out['step'] = {'tracer': [hilo(v) for v in _flat(step)]}
    else:
        tend = lambda s, c=cfg: list(swe_tendency(mesh, s[0], s[1], c))
        k0 = tend([uv, eta])
        k_alt = tend([uv, eta], alt)
        pack = lambda s: {'uv': [hilo(v) for v in _flat(s[0])], 'eta': [hilo(v) for v in _flat(s[1])]}
        out['tendency'] = pack(k0)
        s1 = ssprk33(tend, [uv, eta])
        out['step'] = pack(s1)
        if cfg.get('steps') == 2:
            out['two_steps'] = pack(ssprk33(tend, s1))
    share = _norm_diff(k0, k_alt)
    if share < MIN_SHARE:
        raise SystemExit('case {:}/{:}: share {:.2e} below {:.0e}: a match would be no evidence'.format(mesh.name, name, share, MIN_SHARE))
    out['share'] = share
    return out


# which file holds which cases (group, or case names) and which results: every file stays below 150 KB
RESULTS = ('tendency', 'step', 'two_steps')
FILES = [('exact_weakforms.json', 'tri8', ('walls', 'boundary'), RESULTS),
         ('exact_weakforms_tri8_terms.json', 'tri8', ('source', 'viscosity', 'tracer'), RESULTS),
         ('exact_weakforms_quad4.json', 'quad4', ('walls', 'boundary'), RESULTS),
         ('exact_weakforms_quad4_terms.json', 'quad4', ('source', 'viscosity', 'tracer'), RESULTS),
         ('exact_weakforms_tri345.json', 'tri345', ('combined',), RESULTS),
         ('exact_weakforms_tri345_bare.json', 'tri345', ('bare',), RESULTS),
         ('exact_weakforms_quad72.json', 'quad72', ('combined',), ('tendency', 'step')),
         ('exact_weakforms_quad72_two_steps.json', 'quad72', ('combined',), ('two_steps',))]
MAX_BYTES = 150*1024
_CACHE = {}


def mesh_entry(mesh, state):
    uv, eta, T = state
    return dict(vertices=[list(p) for p in mesh.v], cells=[list(c) for c in mesh.cells], facet_markers=mesh.facet_markers,
                boundary_len=_floats({m: v for m, v in mesh.bnd_len.items()}), uv=_floats(uv), eta=_floats(eta), tracer=_floats(T))


def build_file(fname, only=None, all_meshes=None):
    """the dictionary written to ``fname``; ``only``: compute just these case names"""
    _, mname, groups, results = next(f for f in FILES if f[0] == fname)
    mesh = (all_meshes or meshes())[mname]
    state = mesh_state(mesh, mname)
    doc = dict(format='exact weak forms 1', g_grav=float(G), depth=float(H), rho0=float(RHO0),
               meshes={mname: mesh_entry(mesh, state)}, cases={})
    for name, group, cfg, alt in case_table(mesh, mname):
        if group in groups and (only is None or name in only):
            if (mname, name) not in _CACHE:
                _CACHE[mname, name] = compute_case(mesh, name, cfg, alt, state)
            c = {k_: v for k_, v in _CACHE[mname, name].items() if k_ in results or k_ not in RESULTS}
            c['group'] = group
            doc['cases'][mname + '/' + name] = c
    return doc


def dumps(doc):
    """one line per case: stable bytes, readable diffs"""
    head = {k_: v for k_, v in doc.items() if k_ != 'cases'}
    lines = ['{"cases": {']
    names = sorted(doc['cases'])
    for i, nm in enumerate(names):
        lines.append(json.dumps(nm) + ': ' + json.dumps(doc['cases'][nm], sort_keys=True, separators=(',', ':'))
                     + (',' if i + 1 < len(names) else ''))
    lines.append('},')
    lines.append(json.dumps(head, sort_keys=True, separators=(',', ':'))[1:])
    return '\n'.join(lines) + '\n'


def write_gz(path, text):
    """the JSON text gzip-compressed with a fixed header (no name, no time): the same bytes on every run"""
    with open(path, 'wb') as raw:
        with gzip.GzipFile(filename='', mode='wb', fileobj=raw, mtime=0, compresslevel=9) as fh:
            fh.write(text.encode())


def main():
    ms = meshes()
    for fname in (f[0] for f in FILES):
        text = dumps(build_file(fname, all_meshes=ms))
        assert len(text.encode()) < MAX_BYTES, (fname, len(text))
        write_gz(os.path.join(HERE, fname + '.gz'), text)
        print('{:}.gz {:d} bytes of JSON'.format(fname, len(text)))


if __name__ == '__main__':
    sys.exit(main())
