"""
Smagorinsky eddy viscosity: the numpy restatement of csrc/swe2d_smag.hip, operation by operation.

The closure is the reference's ``SmagorinskyViscosity`` (thetis/utility3d.py:879-997, weak-form gradient), whose formula is
two-dimensional: ``nu = (C_s h)^2 sqrt(D_T^2 + D_S^2)``, ``D_T = du/dx - dv/dy``, ``D_S = du/dy + dv/dx``.  Departures of this
build: the projection onto CG-P1 is LUMPED (no global solve inside the step), and the closure feeds the 2D model's
``horizontal_viscosity`` (the reference wires it into its 3D solver only).

``HostSmagorinsky`` is what a device class without ``smag_set`` runs, step by step on the host, and the yardstick of the kernels:
every sum and product below stands in the order the kernels make it, so the two agree bit for bit.
"""
import numpy as np

from .function import triangle_quadrature

__all__ = ['HostSmagorinsky', 'check_supported', 'vertex_cell_table', 'MAX_H_DIFF_FACTOR']

# alpha of max_h_diff = alpha h^2 / dt (thetis/solver.py:861-864): 1/60/(p (p + 1)) with p = 1
MAX_H_DIFF_FACTOR = 1.0/60.0/(1*(1 + 1))


def check_supported(options, mesh, comm_size=1):
    """what ``options.use_smagorinsky_viscosity`` does not run with, refused by name"""
    if not getattr(options, 'use_smagorinsky_viscosity', False):
        return
    if np.asarray(mesh.cells).shape[1] != 3:
        raise NotImplementedError('use_smagorinsky_viscosity: quadrilaterals are not implemented (the closure runs on triangles)')
    if int(comm_size) > 1:
        raise NotImplementedError('use_smagorinsky_viscosity: several ranks are not implemented (the lumped projection needs every '
                                  'cell of a vertex; run on one device)')
    if getattr(options, 'use_wetting_and_drying', False):
        raise NotImplementedError('use_smagorinsky_viscosity: not together with use_wetting_and_drying')


def vertex_cell_table(cells, n_vertices):
    """CSR table vertex -> (cell << 2 | local node), cells ascending within a vertex: (ptr (V + 1,), idx (3 N,)) as int32"""
    cells = np.asarray(cells, dtype=np.int64)
    n = cells.shape[0]
    ent = ((np.arange(n, dtype=np.int64)[:, None] << 2) | np.arange(3, dtype=np.int64)[None, :]).ravel()
    order = np.argsort(cells.ravel(), kind='stable')         # (stable: ascending cell index within a vertex)
    ptr = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(cells.ravel(), minlength=n_vertices), out=ptr[1:])
    return ptr.astype(np.int32), ent[order].astype(np.int32)


class HostSmagorinsky(object):
    """``mesh``: triangles with ``cells``, ``vertex_xy``, ``cell_nbr`` (neighbour cell, or < 0 on a boundary facet) and
    ``cell_nbr_facet``; facet f of a cell joins its nodes f and f + 1.  ``h_elem``: the CG-P1 element size per vertex (default:
    ``cgproject.elem_size_p1``).  ``max_viscosity``: None = ``MAX_H_DIFF_FACTOR h_v^2 / dt`` with the ``dt`` of the update."""

    def __init__(self, mesh, c_s, h_elem=None, min_val=1e-10, max_viscosity=None):
        cells = np.asarray(mesh.cells)
        if cells.shape[1] != 3:
            raise NotImplementedError('use_smagorinsky_viscosity: quadrilaterals are not implemented')
        self.cells = cells
        self.n_cells, self.n_vertices = cells.shape[0], int(np.asarray(mesh.vertex_xy).shape[0])
        self.c_s = float(c_s)
        self.min_val = float(min_val)
        self.max_viscosity = None if max_viscosity is None else float(max_viscosity)
        if h_elem is None:
            from .cgproject import elem_size_p1
            h_elem = elem_size_p1(mesh)
        self.h_elem = np.ascontiguousarray(h_elem, dtype=np.float64).reshape(self.n_vertices)
        nbr = np.asarray(mesh.cell_nbr)
        self.bnd = nbr < 0                                                   # (N, 3)
        self.nbr = np.where(self.bnd, np.arange(self.n_cells)[:, None], nbr)
        self.nbf = np.where(self.bnd, 0, np.asarray(mesh.cell_nbr_facet))
        xy = np.asarray(mesh.vertex_xy, dtype=np.float64)[cells]            # (N, 3, 2)
        x, y = xy[:, :, 0], xy[:, :, 1]
        det = (x[:, 1] - x[:, 0])*(y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0])*(y[:, 1] - y[:, 0])
        self.area = 0.5*np.abs(det)
        inv = 1.0/det
        # d phi_i / dx, d phi_i / dy
        self.gd = np.stack([np.stack([(y[:, 1] - y[:, 2])*inv, (y[:, 2] - y[:, 0])*inv, (y[:, 0] - y[:, 1])*inv], axis=1),
                            np.stack([(x[:, 2] - x[:, 1])*inv, (x[:, 0] - x[:, 2])*inv, (x[:, 1] - x[:, 0])*inv], axis=1)])
        two_a = 2.0*self.area
        # outward normal times facet length, over 6: facet f lies opposite node f + 2
        self.wf = np.stack([np.stack([-(two_a*self.gd[d][:, (f + 2) % 3])/6.0 for f in range(3)], axis=1) for d in range(2)])
        self.third = self.area/3.0
        self.ptr, self.idx = vertex_cell_table(cells, self.n_vertices)
        self.bary, self.w = triangle_quadrature()
        self.grad = self.moments = self.nu = self.total = None

    def weak_gradient(self, uv):
        """(N, 2, 2, 3): component, direction, node"""
        uv = np.asarray(uv, dtype=np.float64).reshape(self.n_cells, 3, 2)
        n = np.arange(self.n_cells)
        G = np.empty((self.n_cells, 2, 2, 3))
        q = 3.0/self.area
        for c in range(2):
            u = uv[:, :, c]
            ha, hb = [], []
            for f in range(3):
                kn, f2 = self.nbr[:, f], self.nbf[:, f]
                na, nb = u[kn, (f2 + 1) % 3], u[kn, f2]          # the neighbour's trace at my nodes f and f + 1
                ha.append(np.where(self.bnd[:, f], u[n, f], 0.5*(u[n, f] + na)))
                hb.append(np.where(self.bnd[:, f], u[n, (f + 1) % 3], 0.5*(u[n, (f + 1) % 3] + nb)))
            m = self.third*((u[:, 0] + u[:, 1]) + u[:, 2])
            for d in range(2):
                r = [-(self.gd[d][:, i]*m) for i in range(3)]
                for f in range(3):
                    ia, ib = f, (f + 1) % 3
                    r[ia] = r[ia] + self.wf[d][:, f]*(2.0*ha[f] + hb[f])
                    r[ib] = r[ib] + self.wf[d][:, f]*(ha[f] + 2.0*hb[f])
                R = (r[0] + r[1]) + r[2]
                for i in range(3):
                    G[:, c, d, i] = q*(4.0*r[i] - R)
        return G

    def cell_moments(self, G):
        """(N, 3): b_{K,i} = A sum_q w_q lambda_i(q) nu_q"""
        dT = G[:, 0, 0, :] - G[:, 1, 1, :]
        dS = G[:, 0, 1, :] + G[:, 1, 0, :]
        he = self.h_elem[self.cells]
        acc = [np.zeros(self.n_cells) for _ in range(3)]
        for lam, w in zip(self.bary, self.w):
            l0, l1, l2 = (float(v) for v in lam)
            T = (l0*dT[:, 0] + l1*dT[:, 1]) + l2*dT[:, 2]
            S = (l0*dS[:, 0] + l1*dS[:, 1]) + l2*dS[:, 2]
            hq = (l0*he[:, 0] + l1*he[:, 1]) + l2*he[:, 2]
            ch = self.c_s*hq
            nu = (ch*ch)*np.sqrt(T*T + S*S)
            for i, li in enumerate((l0, l1, l2)):
                acc[i] = acc[i] + (float(w)*li)*nu
        return np.stack([self.area*a for a in acc], axis=1)

    def lumped_projection(self, moments, third=None):
        """(V,): sum of the moments of a vertex's (cell, node) pairs over the sum of A/3, cells ascending"""
        third = self.third if third is None else third
        num, den = np.zeros(self.n_vertices), np.zeros(self.n_vertices)
        count = np.diff(self.ptr)
        for j in range(int(count.max()) if len(count) else 0):     # the j-th entry of every vertex that has one
            v = np.nonzero(count > j)[0]
            ent = self.idx[self.ptr[v] + j]
            k, i = ent >> 2, ent & 3
            num[v] = num[v] + moments[k, i]
            den[v] = den[v] + third[k]
        out = np.zeros(self.n_vertices)
        has = count > 0
        out[has] = num[has]/den[has]
        return out

    def max_v(self, dt):
        if self.max_viscosity is not None:
            return np.full(self.n_vertices, self.max_viscosity)
        return (MAX_H_DIFF_FACTOR*(self.h_elem*self.h_elem))/float(dt)

    def update(self, uv, dt, background=0.0):
        """One evaluation from the velocity ``uv`` (N, 3, 2): returns background + clipped viscosity per vertex; ``grad``,
        ``moments``, ``nu`` (clipped, without the background) and ``total`` are kept."""
        self.grad = self.weak_gradient(uv)
        self.moments = self.cell_moments(self.grad)
        nu = self.lumped_projection(self.moments)
        max_v = self.max_v(dt)
        nu = np.where(nu < max_v, nu, max_v)
        nu = np.where(nu > self.min_val, nu, self.min_val)
        self.nu = nu
        self.total = np.asarray(background, dtype=np.float64) + nu
        return self.total
