// swe2d_smag.hip - Smagorinsky eddy viscosity (include/swe2d.h; thetis_amd/smagorinsky.py restates it in numpy, in the
// same operation order): a cell pass - weak velocity gradient in P1(K)^4, the viscosity at the points of the degree-4 rule, the three
// cell moments - and a vertex pass - the lumped projection over a vertex's cells in the order the host lists them, the clip, the
// background - that rewrites the handle's per-vertex viscosity.  FP64, no contraction, no atomics: the same bits whatever the schedule.
#include "swe2d_handle.h"

// the 6-point degree-4 rule of thetis_amd/function.py (triangle_quadrature): barycentric points, weights normalised to sum 1
#define SWE_SMAG_NQ 6
__constant__ double swe_smag_bary[SWE_SMAG_NQ][3] = {
    {0.10810301816807, 0.445948490915965, 0.445948490915965}, {0.445948490915965, 0.10810301816807, 0.445948490915965},
    {0.445948490915965, 0.445948490915965, 0.10810301816807}, {0.816847572980459, 0.091576213509771, 0.091576213509771},
    {0.091576213509771, 0.816847572980459, 0.091576213509771}, {0.091576213509771, 0.091576213509771, 0.816847572980459}};
__constant__ double swe_smag_w[SWE_SMAG_NQ] = {0.22338158967801122, 0.22338158967801122, 0.22338158967801122,
                                               0.1099517436553221, 0.1099517436553221, 0.1099517436553221};

struct SweSmagCellArgs {
    const double *state;                        // buffer A: u0 u1 u2 v0 v1 v2 ...
    const int4 *idxc, *idx4;                    // the packed connectivity (swe_conn_load), or idx4 == null: the planes below
    const int2 *idx2;
    const int *nbr, *cv;
    const double *vx, *vy, *he;                 // per vertex: coordinates, element size
    double *planes;                             // b_0 b_1 b_2 | A/3, [stride] each
    double *grad;                               // debug: the 12 gradient planes [component][direction][node], or null
    size_t stride;
    int n_cells;
    double cs;
};

__global__ void __launch_bounds__(256) swe_smag_cell_kernel(SweSmagCellArgs a)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= a.n_cells) return;
    const size_t S = a.stride;
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    int nb[3], vid[3];
    if (a.idx4) {
        swe_conn_load(a.idxc, a.idx4, a.idx2, k, nb, vid);
    } else {
        const swe_rsrc_t rn = swe_rsrc(a.nbr), rc = swe_rsrc(a.cv);
#pragma unroll
        for (int i = 0; i < 3; i++) { nb[i] = swe_ldi(rn, k4, i*S4); vid[i] = swe_ldi(rc, k4, i*S4); }
    }
    const swe_rsrc_t ru[2] = {swe_rsrc(a.state), swe_rsrc(a.state + 3*S)};
    const swe_rsrc_t rx = swe_rsrc(a.vx), ry = swe_rsrc(a.vy), rh = swe_rsrc(a.he);
    double u[2][3], x[3], y[3], he[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u[0][i] = swe_ld(ru[0], k8, i*S8);
        u[1][i] = swe_ld(ru[1], k8, i*S8);
        x[i] = swe_ld(rx, (unsigned)vid[i]*8u, 0u);
        y[i] = swe_ld(ry, (unsigned)vid[i]*8u, 0u);
        he[i] = swe_ld(rh, (unsigned)vid[i]*8u, 0u);
    }
    // the facet values u_hat at the facet's two nodes: the mean with the neighbour's trace, the own value on a boundary facet
    double ha[2][3], hb[2][3];
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const int nbf = nb[f];
        const bool bnd = nbf < 0;
        const int kn = bnd ? k : (nbf >> 2);
        const int f2 = bnd ? f : (nbf & 3);
        const unsigned kn8 = (unsigned)kn*8u;
        const unsigned ob = kn8 + (f2 == 0 ? 0u : (f2 == 1 ? S8 : 2u*S8));         // node f2 of the neighbour: my node f + 1
        const unsigned oa = kn8 + (f2 == 0 ? S8 : (f2 == 1 ? 2u*S8 : 0u));         // node f2 + 1: my node f
        const int ia = f, ib = (f + 1) % 3;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const double na = swe_ld(ru[c], oa, 0u), nbv = swe_ld(ru[c], ob, 0u);
            ha[c][f] = bnd ? u[c][ia] : 0.5*(u[c][ia] + na);
            hb[c][f] = bnd ? u[c][ib] : 0.5*(u[c][ib] + nbv);
        }
    }
    const double det = (x[1] - x[0])*(y[2] - y[0]) - (x[2] - x[0])*(y[1] - y[0]);
    const double A = 0.5*__builtin_fabs(det);
    const double inv = 1.0/det;
    double gd[2][3];                                                               // d phi_i / dx, d phi_i / dy
    gd[0][0] = (y[1] - y[2])*inv; gd[0][1] = (y[2] - y[0])*inv; gd[0][2] = (y[0] - y[1])*inv;
    gd[1][0] = (x[2] - x[1])*inv; gd[1][1] = (x[0] - x[2])*inv; gd[1][2] = (x[1] - x[0])*inv;
    const double twoA = 2.0*A, third = A/3.0, q = 3.0/A;
    double wf[2][3];                                                               // outward normal times facet length, over 6
#pragma unroll
    for (int f = 0; f < 3; f++) {
        wf[0][f] = -(twoA*gd[0][(f + 2) % 3])/6.0;
        wf[1][f] = -(twoA*gd[1][(f + 2) % 3])/6.0;
    }
    double G[2][2][3];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const double m = third*((u[c][0] + u[c][1]) + u[c][2]);
#pragma unroll
        for (int d = 0; d < 2; d++) {
            double r[3];
#pragma unroll
            for (int i = 0; i < 3; i++) r[i] = -(gd[d][i]*m);
#pragma unroll
            for (int f = 0; f < 3; f++) {
                const int ia = f, ib = (f + 1) % 3;
                r[ia] = r[ia] + wf[d][f]*(2.0*ha[c][f] + hb[c][f]);
                r[ib] = r[ib] + wf[d][f]*(ha[c][f] + 2.0*hb[c][f]);
            }
            const double R = (r[0] + r[1]) + r[2];
#pragma unroll
            for (int i = 0; i < 3; i++) G[c][d][i] = q*(4.0*r[i] - R);
        }
    }
    if (a.grad) {
#pragma unroll
        for (int p = 0; p < 12; p++) swe_st(swe_rsrc(a.grad + (size_t)p*S), k8, 0u, G[p/6][(p/3) % 2][p % 3]);
    }
    double dT[3], dS[3], acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++) { dT[i] = G[0][0][i] - G[1][1][i]; dS[i] = G[0][1][i] + G[1][0][i]; }
#pragma unroll
    for (int p = 0; p < SWE_SMAG_NQ; p++) {
        const double l0 = swe_smag_bary[p][0], l1 = swe_smag_bary[p][1], l2 = swe_smag_bary[p][2], w = swe_smag_w[p];
        const double T = (l0*dT[0] + l1*dT[1]) + l2*dT[2];
        const double Sq = (l0*dS[0] + l1*dS[1]) + l2*dS[2];
        const double hq = (l0*he[0] + l1*he[1]) + l2*he[2];
        const double ch = a.cs*hq;
        const double nu = (ch*ch)*sqrt(T*T + Sq*Sq);
        acc[0] = acc[0] + (w*l0)*nu;
        acc[1] = acc[1] + (w*l1)*nu;
        acc[2] = acc[2] + (w*l2)*nu;
    }
    const swe_rsrc_t ro = swe_rsrc(a.planes), rt = swe_rsrc(a.planes + 3*S);
#pragma unroll
    for (int i = 0; i < 3; i++) swe_st(ro, k8, i*S8, A*acc[i]);
    swe_st(rt, k8, 0u, third);
}

struct SweSmagVertexArgs {
    const int *off, *ent;                       // vertex -> (cell << 2 | local node), in the order the host listed them
    const double *planes;                       // b_0 b_1 b_2 | A/3
    const double *he;
    const double *bg_v;                         // the background viscosity per vertex, or null: bg_const
    double *nu_clip, *nu_total;
    size_t stride;
    int n_vertices;
    double bg_const, min_val, max_const, dt;
};

__global__ void __launch_bounds__(256) swe_smag_vertex_kernel(SweSmagVertexArgs a)
{
#pragma clang fp contract(off)
    const int v = blockIdx.x*256 + threadIdx.x;
    if (v >= a.n_vertices) return;
    const unsigned S8 = (unsigned)a.stride*8u, v8 = (unsigned)v*8u;
    const swe_rsrc_t rl = swe_rsrc(a.off), rn = swe_rsrc(a.ent), rb = swe_rsrc(a.planes), rt = swe_rsrc(a.planes + 3*a.stride);
    const int e0 = swe_ldi(rl, (unsigned)v*4u, 0u), e1 = swe_ldi(rl, (unsigned)v*4u, 4u);
    double num = 0.0, den = 0.0;
    for (int e = e0; e < e1; e++) {
        const int ent = swe_ldi(rn, (unsigned)e*4u, 0u);
        const unsigned k8 = (unsigned)(ent >> 2)*8u;
        num = num + swe_ld(rb, k8, (unsigned)(ent & 3)*S8);
        den = den + swe_ld(rt, k8, 0u);
    }
    double nu = e1 > e0 ? num/den : 0.0;
    const double hv = swe_ld(swe_rsrc(a.he), v8, 0u);
    const double max_v = a.max_const >= 0.0 ? a.max_const : ((1.0/60.0/2.0)*(hv*hv))/a.dt;
    nu = nu < max_v ? nu : max_v;
    nu = nu > a.min_val ? nu : a.min_val;
    const double bg = a.bg_v ? swe_ld(swe_rsrc(a.bg_v), v8, 0u) : a.bg_const;
    swe_st(swe_rsrc(a.nu_clip), v8, 0u, nu);
    swe_st(swe_rsrc(a.nu_total), v8, 0u, bg + nu);
}

namespace {

int smag_check(Handle *h, const char *who)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->smag.on) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle has no Smagorinsky viscosity (swe2d_smag_set)");
    return SWE2D_OK;
}

void smag_release(Handle *h)
{
    Handle::Smag &s = h->smag;
    if (s.on) {
        // the caller's viscosity takes its place again
        h->nu_v = std::move(s.bg_v);
        h->nu_const = s.bg_const;
        h->visc = s.visc_caller;
    }
    s = Handle::Smag();
}

int smag_cell_launch(Handle *h, bool with_gradient)
{
    const Handle::Smag &s = h->smag;
    SweSmagCellArgs a{};
    a.state = h->state[0];
    a.idxc = h->idxc; a.idx4 = h->idx4; a.idx2 = h->idx2;
    a.nbr = h->nbr; a.cv = h->cv;
    a.vx = h->vx; a.vy = h->vy; a.he = s.he;
    a.planes = s.planes;
    a.grad = with_gradient ? s.grad : nullptr;
    a.stride = h->stride;
    a.n_cells = h->n_cells;
    a.cs = s.cs;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_smag_cell_kernel, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

}  // namespace

int swe2d_impl::smag_update_launch(Handle *h)
{
    const Handle::Smag &s = h->smag;
    if (int rc = smag_cell_launch(h, false)) return rc;
    SweSmagVertexArgs a{};
    a.off = s.off; a.ent = s.ent;
    a.planes = s.planes;
    a.he = s.he;
    a.bg_v = s.bg_v;
    a.nu_clip = s.nu_clip; a.nu_total = h->nu_v;
    a.stride = h->stride;
    a.n_vertices = h->n_vertices;
    a.bg_const = s.bg_const; a.min_val = s.min_val; a.max_const = s.max_const;
    a.dt = h->par.dt;                                  // (read at every launch: swe2d_set_dt needs no upload)
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_smag_vertex_kernel, dim3(grid_for(h->n_vertices)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

extern "C" {

int swe2d_smag_set(swe2d_handle *hh, double c_s, const double *h_elem_vertex, double min_val, double max_const_or_negative,
                   const int32_t *vertex_cell_ptr, const int32_t *vertex_cell_idx)
{
    Handle *h = H(hh);
    if (!h || !h_elem_vertex || !vertex_cell_ptr || !vertex_cell_idx) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: null argument");
    if (h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_set: the Smagorinsky viscosity runs on triangles only (no quadrilaterals)");
    if (h->n_owned != h->n_cells) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_set: the Smagorinsky viscosity is not available on partitions");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_set: not with wetting-drying");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_set inside a stream capture");
    if (!(c_s >= 0.0) || !std::isfinite(c_s) || !(min_val >= 0.0) || !std::isfinite(min_val) || std::isnan(max_const_or_negative))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: c_s and min_val must be finite and >= 0, the maximum a number");
    const int n = h->n_cells, nv = h->n_vertices;
    for (int v = 0; v < nv; v++)
        if (!std::isfinite(h_elem_vertex[v]))       // (the consistent P1 projection of the cell size may undershoot 0 on a graded mesh: only its square enters)
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: the element size must be finite");
    // the table lists every (cell, node) pair once, under the node's vertex
    if (vertex_cell_ptr[0] != 0 || (long long)vertex_cell_ptr[nv] != 3ll*n || h->host_cells.size() != (size_t)3*n)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: the vertex table must hold 3*n_cells entries");
    for (int v = 0; v < nv; v++) {
        if (vertex_cell_ptr[v + 1] < vertex_cell_ptr[v]) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: the vertex table's offsets must not decrease");
        for (int e = vertex_cell_ptr[v]; e < vertex_cell_ptr[v + 1]; e++) {
            const int k = vertex_cell_idx[e] >> 2, i = vertex_cell_idx[e] & 3;
            if (vertex_cell_idx[e] < 0 || k >= n || i >= 3 || h->host_cells[(size_t)3*k + i] != v)
                return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_set: an entry of the vertex table is not a node of its vertex");
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Handle::Smag &s = h->smag;
    const size_t S = h->stride;
    if (!s.on) {
        // the caller's viscosity becomes the background, in a buffer of its own: nu_v is rewritten at every step
        DevArray<double> total;
        HIP_TRY(h, total.alloc(nv));
        s.visc_caller = h->visc;
        if (h->visc) s.bg_v = std::move(h->nu_v);          // (the array of a viscosity that was switched off goes with the next line)
        s.bg_const = h->visc ? h->nu_const : 0.0;
        h->nu_v = std::move(total);
        h->visc = true;
        s.on = true;
    }
    HIP_TRY(h, s.he.ensure(nv));
    HIP_TRY(h, s.off.ensure((size_t)(nv + 1)));
    HIP_TRY(h, s.ent.ensure((size_t)3*n));
    HIP_TRY(h, s.planes.ensure(4*S));
    HIP_TRY(h, s.nu_clip.ensure(nv));
    HIP_TRY(h, hipMemcpyAsync(s.he, h_elem_vertex, (size_t)nv*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(s.off, vertex_cell_ptr, (size_t)(nv + 1)*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(s.ent, vertex_cell_idx, (size_t)3*n*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(s.planes, 0, 4*S*sizeof(double), h->stream));
    HIP_TRY(h, hipMemsetAsync(s.nu_clip, 0, (size_t)nv*sizeof(double), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    s.cs = c_s; s.min_val = min_val; s.max_const = max_const_or_negative;
    // nu_v holds a viscosity from here on: the one of the state that is there
    return smag_update_launch(h);
}

int swe2d_smag_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->smag.on) return SWE2D_OK;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_clear inside a stream capture");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    smag_release(h);
    return SWE2D_OK;
}

int swe2d_smag_update(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = smag_check(h, "swe2d_smag_update")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return smag_update_launch(h);
}

int swe2d_smag_read(swe2d_handle *hh, int which, double *out)
{
    Handle *h = H(hh);
    if (int rc = smag_check(h, "swe2d_smag_read")) return rc;
    if (!out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_read: null argument");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_smag_read inside a stream capture");
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Smag &s = h->smag;
    const size_t S = h->stride, n = (size_t)h->n_cells, nv = (size_t)h->n_vertices;
    switch (which) {
    case SWE2D_SMAG_GRADIENT:
        // the debug flag: the cell pass once more on the state that is there, with the 12 gradient planes written
        HIP_TRY(h, s.grad.ensure(12*S));
        HIP_TRY(h, s.grad_out.ensure(12*n));
        if (int rc = smag_cell_launch(h, true)) return rc;
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, s.grad, s.grad_out, S, h->n_cells, 12);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(out, s.grad_out, 12*n*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        break;
    case SWE2D_SMAG_MOMENTS:
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, s.planes, h->stage_eta, S, h->n_cells, 3);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(out, h->stage_eta, 3*n*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        break;
    case SWE2D_SMAG_NU:
        HIP_TRY(h, hipMemcpyAsync(out, s.nu_clip, nv*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        break;
    case SWE2D_SMAG_TOTAL:
        HIP_TRY(h, hipMemcpyAsync(out, h->nu_v, nv*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        break;
    default:
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_smag_read: unknown quantity");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

}  // extern "C"
