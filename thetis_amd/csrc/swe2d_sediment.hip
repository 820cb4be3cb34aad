// swe2d_sediment.hip - suspended sediment and Exner bed evolution: the swe2d_sediment_* / swe2d_exner_* entry points and their four
// passes.  The sediment field is one of the handle's tracers; what is new is where its source comes from and what it does to the bed.
//
// swe_sediment_coeff_kernel   - once per time step, one lane per cell: the closures of the sediment model (thetis_amd/sediment_model.py
//                               restates them in numpy; include/swe2d.h has the formulas) at the cell's three DG nodes from its own
//                               nodal uv and H.  Written: three nodal planes each of the erosion flux E, the deposition coefficient D and
//                               the equilibrium concentration E/D.  The only pass with real arithmetic: 4 logarithms, 1 power and 2
//                               square roots per node from the device's math library; every branch of the closures is a select.
// swe_sediment_bc_kernel      - with it, one lane per boundary cell: the equilibrium plane (times the nodal depth in the conservative
//                               form) into the sediment tracer's per-facet value table, on the facets of 'equilibrium' markers.
// swe_sediment_source_kernel  - in front of every stage launch of the sediment tracer, over that launch's cell range (the seam of the
//                               reaction pass): s = (E - D*S)/H, conservative E - (D*q)/H, S the stage's input buffer.
// swe_exner_kernel            - after the sediment step, one lane per vertex: a gather over the vertex's (cell, local node) list in
//                               ascending cell order of  A/12 (2 r_i + r_j + r_k)  and  A/3,  r = E - D*S the net erosion at the nodes.
//                               The new bed goes to a second array and is copied over the old one afterwards: in the conservative form r
//                               reads the depth, i.e. the bed of OTHER vertices.  No atomics but the counter of vertices left unchanged.
// The last three are + - * / in a fixed order without contraction: thetis_amd/sediment_model.py (HostSediment) gives their bits from the
// same planes.  All loads and stores of a lane are its own cell's / vertex's; plane accesses are coalesced, the gather is not.
#include "swe2d_handle.h"

struct SweSedArgs {
    const double *state;                        // buffer A: u [3][S] | v [3][S] | eta [3][S]
    const double *tin;                          // source pass / Exner: the sediment tracer's buffer
    const int *cv, *nbr;
    const double *vh;
    double *planes;                             // E [3][S] | D [3][S] | equilibrium [3][S]
    double *out;                                // source planes / per-facet value table / new bed
    const int *list;                            // boundary cells | CSR offsets
    const int *ent;                             // CSR entries: cell << 2 | local node
    const double *area;                         // [n_cells]
    unsigned *count;
    size_t stride;
    int begin, end;                             // cell range / list length / vertices
    int nonlinear, conservative;
    unsigned eq_markers;
    double dtf, min_depth;                      // Exner: dt*fac, the floor of the depth
    swe2d_sediment_params par;
};

// the closures at one node (include/swe2d.h, swe2d_sediment_params); no argument of log / pow / sqrt leaves its domain on any branch
__device__ __forceinline__ void swe_sediment_closures(const swe2d_sediment_params &p, double u, double v, double H,
                                                      double &E, double &D, double &ceq)
{
#pragma clang fp contract(off)
    const double unorm = u*u + v*v;
    const double hc = H > 0.001 ? H : 0.001;
    const double ax = 11.036*hc/p.ks;
    const double aux = ax > 1.001 ? ax : 1.001;
    const double lq = log(aux)/p.kappa;
    const double qfc = 2.0/(lq*lq);
    const bool deep = H > p.ksp;
    const double lc = (1.0/p.kappa)*log(11.036*(deep ? H : p.ksp)/p.ksp);
    const double cfactor = deep ? 2.0/(lc*lc) : 0.0;
    const double mu = qfc > 0.0 ? cfactor/qfc : 0.0;
    const double B = p.a > H ? 1.0 : p.a/H;
    const double ustar = sqrt(0.5*qfc*unorm);
    const double rouse = p.ws/(p.kappa*ustar) - 1.0;                       // (still water: +inf, the minimum below takes 3)
    const double rm = rouse < 3.0 ? rouse : 3.0;
    const double step = __builtin_fabs(rouse) > 1e-4 ? B*(1.0 - pow(B, rm))/rm : -B*log(B);
    const double ir0 = step > 1e-12 ? 1.0/step : 1e12;
    const double ir = ir0 > 1.0 ? ir0 : 1.0;
    const double tau = p.rho0*0.5*qfc*unorm*mu;
    const double T = tau > 0.0 ? (tau - p.taucr)/p.taucr : -1.0;
    const double T15 = T > 0.0 ? T*sqrt(T) : 0.0;
    E = p.ws*(p.erosion_factor*T15);
    D = p.ws*ir;
    ceq = E/D;
}

__global__ void __launch_bounds__(256) swe_sediment_coeff_kernel(SweSedArgs a)
{
#pragma clang fp contract(off)
    const int k = a.begin + blockIdx.x*256 + threadIdx.x;
    if (k >= a.end) return;
    const size_t S = a.stride;
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t ru = swe_rsrc(a.state), rv = swe_rsrc(a.state + 3*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv),
                     rh = swe_rsrc(a.vh);
    const swe_rsrc_t oE = swe_rsrc(a.planes), oD = swe_rsrc(a.planes + 3*S), oQ = swe_rsrc(a.planes + 6*S);
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
        const double u = swe_ld(ru, k8, i*S8), v = swe_ld(rv, k8, i*S8), eta = swe_ld(re, k8, i*S8);
        const double h = swe_ld(rh, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
        const double H = a.nonlinear ? eta + h : h;
        double E, D, ceq;
        swe_sediment_closures(a.par, u, v, H, E, D, ceq);
        swe_st(oE, k8, i*S8, E);
        swe_st(oD, k8, i*S8, D);
        swe_st(oQ, k8, i*S8, ceq);
    }
}

__global__ void __launch_bounds__(256) swe_sediment_bc_kernel(SweSedArgs a)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x*256 + threadIdx.x;
    if (j >= a.end) return;
    const size_t S = a.stride;
    const int k = a.list[j];
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t rq = swe_rsrc(a.planes + 6*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv), rh = swe_rsrc(a.vh),
                     rn = swe_rsrc(a.nbr);
    double val[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        val[i] = swe_ld(rq, k8, i*S8);
        if (a.conservative) {
            const double h = swe_ld(rh, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
            const double H = a.nonlinear ? swe_ld(re, k8, i*S8) + h : h;
            val[i] = val[i]*H;
        }
    }
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const int code = swe_ldi(rn, k4, f*S4);
        if (code >= 0 || !((a.eq_markers >> (-code)) & 1u)) continue;
        const swe_rsrc_t ro = swe_rsrc(a.out + (size_t)(3*f)*S);              // plane 3 f + i: node i of the cell for its facet f
#pragma unroll
        for (int i = 0; i < 3; i++) swe_st(ro, k8, i*S8, val[i]);
    }
}

__global__ void __launch_bounds__(256) swe_sediment_source_kernel(SweSedArgs a)
{
#pragma clang fp contract(off)
    const int k = a.begin + blockIdx.x*256 + threadIdx.x;
    if (k >= a.end) return;
    const size_t S = a.stride;
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t rE = swe_rsrc(a.planes), rD = swe_rsrc(a.planes + 3*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv),
                     rh = swe_rsrc(a.vh), rt = swe_rsrc(a.tin), ro = swe_rsrc(a.out);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double E = swe_ld(rE, k8, i*S8), D = swe_ld(rD, k8, i*S8), c = swe_ld(rt, k8, i*S8);
        const double h = swe_ld(rh, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
        const double H = a.nonlinear ? swe_ld(re, k8, i*S8) + h : h;
        swe_st(ro, k8, i*S8, a.conservative ? E - (D*c)/H : (E - D*c)/H);
    }
}

__global__ void __launch_bounds__(256) swe_exner_kernel(SweSedArgs a)
{
#pragma clang fp contract(off)
    const int v = blockIdx.x*256 + threadIdx.x;
    if (v >= a.end) return;
    const size_t S = a.stride;
    const unsigned S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t rE = swe_rsrc(a.planes), rD = swe_rsrc(a.planes + 3*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv),
                     rh = swe_rsrc(a.vh), rt = swe_rsrc(a.tin), rl = swe_rsrc(a.list), rn = swe_rsrc(a.ent), ra = swe_rsrc(a.area);
    const int e0 = swe_ldi(rl, (unsigned)v*4u, 0u), e1 = swe_ldi(rl, (unsigned)v*4u, 4u);
    const double b_old = swe_ld(rh, (unsigned)v*8u, 0u);
    double num = 0.0, den = 0.0, eta_min = 1e300;
    for (int e = e0; e < e1; e++) {
        const int ent = swe_ldi(rn, (unsigned)e*4u, 0u);
        const int k = ent >> 2, i = ent & 3;
        const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u;
        double r[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double E = swe_ld(rE, k8, j*S8), D = swe_ld(rD, k8, j*S8), c = swe_ld(rt, k8, j*S8);
            if (a.conservative) {
                const double h = swe_ld(rh, (unsigned)swe_ldi(rc, k4, j*S4)*8u, 0u);
                const double H = a.nonlinear ? swe_ld(re, k8, j*S8) + h : h;
                r[j] = E - (D*c)/H;
            } else {
                r[j] = E - D*c;
            }
        }
        const double ri = i == 0 ? r[0] : (i == 1 ? r[1] : r[2]);
        const double rj = i == 0 ? r[1] : (i == 1 ? r[2] : r[0]);
        const double rk = i == 0 ? r[2] : (i == 1 ? r[0] : r[1]);
        const double A = swe_ld(ra, k8, 0u);
        num = num + (A/12.0)*((2.0*ri + rj) + rk);
        den = den + A/3.0;
        const double eta = swe_ld(re, k8, (unsigned)i*S8);
        eta_min = eta < eta_min ? eta : eta_min;
    }
    double b_new = b_old;
    if (e1 > e0) {
        const double b = b_old + (a.dtf*num)/den;
        // the shallowest depth the DG elevation gives at this vertex on the new bed (linear equations: the bed itself)
        const double Hmin = a.nonlinear ? eta_min + b : b;
        if (Hmin >= a.min_depth) b_new = b;
        else atomicAdd(a.count, 1u);
    }
    swe_st(swe_rsrc(a.out), (unsigned)v*8u, 0u, b_new);
}

namespace {

int sediment_check(Handle *h, const char *who)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->sed.on) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle has no sediment model (swe2d_sediment_set)");
    return SWE2D_OK;
}

void sediment_fill(Handle *h, SweSedArgs &a)
{
    a.state = h->state[0];
    a.cv = h->cv; a.nbr = h->nbr; a.vh = h->vh;
    a.planes = h->sed.planes;
    a.stride = h->stride;
    a.nonlinear = h->par.use_nonlinear_equations ? 1 : 0;
    a.conservative = h->sed.par.conservative ? 1 : 0;
    a.par = h->sed.par;
}

void sediment_release_tables(Handle *h)
{
    Handle::Sediment &s = h->sed;
    void *ptrs[] = {s.v_off, s.v_ent, s.area, s.vh_new, s.count};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    s.v_off = s.v_ent = nullptr; s.area = s.vh_new = nullptr; s.count = nullptr;
}

void sediment_release(Handle *h)
{
    Handle::Sediment &s = h->sed;
    void *ptrs[] = {s.planes, s.v_off, s.v_ent, s.area, s.vh_new, s.count};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    s = Handle::Sediment();
}

// triangle areas as HostSediment forms them: 0.5*|(x1 - x0)*(y2 - y0) - (x2 - x0)*(y1 - y0)|, no contraction
void sediment_areas(const Handle *h, const double *vx, const double *vy, std::vector<double> &area)
{
#pragma clang fp contract(off)
    const int n = h->n_cells;
    area.resize(n);
    for (int k = 0; k < n; k++) {
        const int *c = &h->host_cells[(size_t)3*k];
        const double ax = vx[c[1]] - vx[c[0]], ay = vy[c[1]] - vy[c[0]], bx = vx[c[2]] - vx[c[0]], by = vy[c[2]] - vy[c[0]];
        const double p = ax*by, q = bx*ay;
        area[k] = 0.5*std::fabs(p - q);
    }
}

}  // namespace

int swe2d_impl::sediment_source_launch(Handle *h, int in, int c0, int c1)
{
    if (c1 <= c0) return SWE2D_OK;
    Handle::Tracer &t = h->tracers[h->sed.tracer];
    SweSedArgs a{};
    sediment_fill(h, a);
    a.tin = t.buf[in];
    a.out = t.source;
    a.begin = c0; a.end = c1;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_sediment_source_kernel, dim3(grid_for(c1 - c0)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

int swe2d_impl::sediment_update_launch(Handle *h)
{
    SweSedArgs a{};
    sediment_fill(h, a);
    a.begin = 0; a.end = h->n_cells;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_sediment_coeff_kernel, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    if (h->sed.eq_markers && h->n_bnd > 0) {
        a.list = h->bnd_cells;
        a.end = h->n_bnd;
        a.eq_markers = h->sed.eq_markers;
        a.out = h->tracers[h->sed.tracer].bc_value_f;
        SWE_CHK_SYNC(h->stream);
        hipLaunchKernelGGL(swe_sediment_bc_kernel, dim3(grid_for(h->n_bnd)), dim3(256), 0, h->stream, a);
        HIP_TRY(h, hipGetLastError());
    }
    return SWE2D_OK;
}

int swe2d_impl::exner_launch(Handle *h)
{
    Handle::Sediment &s = h->sed;
    SweSedArgs a{};
    sediment_fill(h, a);
    a.tin = h->tracers[s.tracer].buf[0];
    a.list = s.v_off; a.ent = s.v_ent; a.area = s.area;
    a.out = s.vh_new;
    a.count = s.count;
    a.begin = 0; a.end = h->n_vertices;
    a.dtf = h->par.dt*s.par.fac;
    a.min_depth = s.par.min_depth;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_exner_kernel, dim3(grid_for(h->n_vertices)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->vh, s.vh_new, (size_t)h->n_vertices*sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return SWE2D_OK;
}

void swe2d_impl::sediment_free(Handle *h) { sediment_release(h); }

extern "C" {

int swe2d_sediment_set(swe2d_handle *hh, int tracer_id, const swe2d_sediment_params *par)
{
    Handle *h = H(hh);
    if (!h || !par) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: null argument");
    if (tracer_id < 0 || tracer_id >= (int)h->tracers.size()) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: unknown tracer id");
    if (h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_sediment_set: the sediment model runs on triangles only");
    if (h->n_owned != h->n_cells) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_sediment_set: the sediment model is not available on partitions");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_sediment_set: not with wetting-drying (the depth planes are tied to the bed)");
    if (par->solve_exner && h->n_farms > 0)
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_sediment_set: solve_exner is not available together with tidal turbine farms");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_sediment_set inside a stream capture");
    const double pos[] = {par->ws, par->dstar, par->taucr, par->a, par->ksp, par->ks, par->rho0, par->kappa, par->fac, par->min_depth};
    for (double x : pos)
        if (!(x > 0.0) || !std::isfinite(x)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: every parameter but erosion_factor must be positive and finite");
    if (!(par->erosion_factor >= 0.0) || !std::isfinite(par->erosion_factor))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: erosion_factor must be >= 0");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->sed.on && h->sed.tracer != tracer_id) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: the handle has a sediment field already (swe2d_sediment_clear)");
    Handle::Tracer &t = h->tracers[tracer_id];
    Handle::Sediment &s = h->sed;
    const size_t S = h->stride, plane_bytes = 3*S*sizeof(double);
    const int n = h->n_cells, nv = h->n_vertices;
    if (!s.planes) {
        HIP_TRY(h, hipMalloc(&s.planes, 3*plane_bytes));
        HIP_TRY(h, hipMemsetAsync(s.planes, 0, 3*plane_bytes, h->stream));
    }
    if (!s.on && (t.source || t.rx.n_code > 0))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: the tracer has a source or a reaction program already (remove it first)");
    if (!t.source) {
        HIP_TRY(h, hipMalloc(&t.source, plane_bytes));
        HIP_TRY(h, hipMemsetAsync(t.source, 0, plane_bytes, h->stream));
    }
    if (!s.count) {                                    // (count is allocated last: a failed attempt is released and built again)
        sediment_release_tables(h);
        // vertex -> (cell, local node), cells ascending; triangle areas
        std::vector<int> off(nv + 1, 0);
        for (size_t j = 0; j < (size_t)3*n; j++) off[h->host_cells[j] + 1]++;
        for (int v = 0; v < nv; v++) off[v + 1] += off[v];
        std::vector<int> ent((size_t)3*n), pos_(off.begin(), off.end() - 1);
        for (int k = 0; k < n; k++)
            for (int i = 0; i < 3; i++) ent[pos_[h->host_cells[(size_t)3*k + i]]++] = (k << 2) | i;
        std::vector<double> vx(nv), vy(nv), area;
        HIP_TRY(h, hipMemcpy(vx.data(), h->vx, (size_t)nv*sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(vy.data(), h->vy, (size_t)nv*sizeof(double), hipMemcpyDeviceToHost));
        sediment_areas(h, vx.data(), vy.data(), area);
        HIP_TRY(h, hipMalloc(&s.v_off, off.size()*sizeof(int)));
        HIP_TRY(h, hipMalloc(&s.v_ent, ent.size()*sizeof(int)));
        HIP_TRY(h, hipMalloc(&s.area, (size_t)n*sizeof(double)));
        HIP_TRY(h, hipMalloc(&s.vh_new, (size_t)nv*sizeof(double)));
        HIP_TRY(h, hipMemcpy(s.v_off, off.data(), off.size()*sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(s.v_ent, ent.data(), ent.size()*sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(s.area, area.data(), (size_t)n*sizeof(double), hipMemcpyHostToDevice));
        unsigned *cnt = nullptr;
        HIP_TRY(h, hipMalloc(&cnt, sizeof(unsigned)));
        if (hipMemset(cnt, 0, sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(cnt); return fail(h, SWE2D_ERR_HIP, "swe2d_sediment_set: clearing the counter failed"); }
        s.count = cnt;
    }
    s.par = *par;
    s.tracer = tracer_id;
    s.on = true;
    t.conservative = par->conservative != 0;
    return SWE2D_OK;
}

int swe2d_sediment_set_equilibrium_bc(swe2d_handle *hh, int marker, int on)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_sediment_set_equilibrium_bc")) return rc;
    if (marker <= 0 || marker >= SWE2D_MAX_MARKERS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "marker out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Tracer &t = h->tracers[h->sed.tracer];
    if (on) {
        if (!t.bc_value_f) {
            const size_t bytes = (size_t)9*h->stride*sizeof(double);
            HIP_TRY(h, hipMalloc(&t.bc_value_f, bytes));
            HIP_TRY(h, hipMemsetAsync(t.bc_value_f, 0, bytes, h->stream));
        }
        h->sed.eq_markers |= 1u << marker;
        t.bc_has_value[marker] = 2;
    } else if ((h->sed.eq_markers >> marker) & 1u) {
        h->sed.eq_markers &= ~(1u << marker);
        t.bc_has_value[marker] = 0;
    }
    return SWE2D_OK;
}

int swe2d_sediment_update(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_sediment_update")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return sediment_update_launch(h);
}

int swe2d_sediment_read(swe2d_handle *hh, double *erosion, double *deposition, double *equilibrium)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_sediment_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    double *dst[3] = {erosion, deposition, equilibrium};
    for (int q = 0; q < 3; q++) {
        if (!dst[q]) continue;
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                           h->sed.planes + (size_t)3*q*h->stride, h->stage_eta, h->stride, h->n_cells, 3);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(dst[q], h->stage_eta, (size_t)3*h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SWE2D_OK;
}

int swe2d_sediment_read_bc(swe2d_handle *hh, double *facet_nodal)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_sediment_read_bc")) return rc;
    if (!facet_nodal) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    const double *tab = h->tracers[h->sed.tracer].bc_value_f;
    if (!tab) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_read_bc: the sediment tracer has no per-facet value table");
    HIP_TRY(h, hipSetDevice(h->device));
    for (int f = 0; f < 3; f++) {
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                           tab + (size_t)3*f*h->stride, h->stage_eta, h->stride, h->n_cells, 3);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(facet_nodal + (size_t)3*f*h->n_cells, h->stage_eta, (size_t)3*h->n_cells*sizeof(double),
                                  hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SWE2D_OK;
}

int swe2d_sediment_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->sed.on) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Handle::Tracer &t = h->tracers[h->sed.tracer];
    for (int m = 1; m < SWE2D_MAX_MARKERS; m++)
        if ((h->sed.eq_markers >> m) & 1u) t.bc_has_value[m] = 0;
    if (t.source) { HIP_TRY(h, hipFree(t.source)); t.source = nullptr; }       // (allocated by swe2d_sediment_set: it refuses a tracer with one)
    t.conservative = false;
    sediment_release(h);
    return SWE2D_OK;
}

int swe2d_exner_step(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_exner_step")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return exner_launch(h);
}

int swe2d_exner_skipped(swe2d_handle *hh, int64_t *n_skipped)
{
    Handle *h = H(hh);
    if (int rc = sediment_check(h, "swe2d_exner_skipped")) return rc;
    if (!n_skipped) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned c = 0;
    HIP_TRY(h, hipMemcpyAsync(&c, h->sed.count, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_skipped = (int64_t)c;
    return SWE2D_OK;
}

int swe2d_set_bathymetry(swe2d_handle *hh, const double *vertex_values)
{
    Handle *h = H(hh);
    if (!h || !vertex_values) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_set_bathymetry: not with wetting-drying (the depth planes are tied to the bed)");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_set_bathymetry inside a stream capture");
    for (int i = 0; i < h->n_vertices; i++)
        if (!std::isfinite(vertex_values[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_set_bathymetry: the bathymetry must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->vh, vertex_values, (size_t)h->n_vertices*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

int swe2d_get_bathymetry(swe2d_handle *hh, double *vertex_values)
{
    Handle *h = H(hh);
    if (!h || !vertex_values) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(vertex_values, h->vh, (size_t)h->n_vertices*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

}  // extern "C"
