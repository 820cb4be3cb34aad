// swe2d_atm.hip - atmospheric forcing from a record of snapshots: the swe2d_atm_* entry points and the evaluation kernel.
//
//     u = (1 - alpha)*u_j + alpha*u_{j+1}     (v, p alike)     alpha = (t - t_j)/(t_{j+1} - t_j)      (thetis/interpolation.py:818-823)
//     m = sqrt(u*u + v*v)      tau = C_D(m)*rho_air*m      tau_x = tau*u      tau_y = tau*v            (thetis/forcing.py:19-79)
//
// The record holds 10 m wind and mean-sea-level pressure per mesh vertex and snapshot, the values of a vertex interleaved:
// tab[snapshot][vertex][W], W = 2 (wind only: u, v), 1 (pressure only) or 3 (u, v, p).  A lane's gather of one snapshot is W
// neighbouring doubles - one cache line, rarely two - instead of W lines of W snapshot-major planes; a record with one quantity
// carries nothing of the other.  swe_atm_kernel - one lane per node value, the node uniform per workgroup, as swe_stats_kernel -
// reads the node's vertex from h->cv, gathers the two snapshots that bracket the time and writes the wind-stress planes
// (component-major, as swe_vertex_to_planes) and the pressure planes of ALL cells, ghosts included: no LDS, no atomics, one writer per
// value.  A vertex is recomputed by every cell that touches it - one launch per stage instead of two.  The bracket j and alpha are
// found on the host (atm_bracket, from its copy of the times) and travel in the kernel arguments; the device searches nothing and
// evaluates no transcendental.  The expressions are formed left to right without contraction: the same in numpy
// (forcing.compute_wind_stress, AtmosphericForcing.set_fields) has the same bits but for the square root's rounding.
#include "swe2d_handle.h"

struct SweAtmArgs {
    const double *s0, *s1;                      // snapshots j and j + 1: [n_vertices][W]
    const int *cv;                              // [NPC][stride] cell vertices
    double *wind, *patm;                        // [2*NPC][stride], [NPC][stride]
    size_t stride;
    double alpha;
    int n_cells, method, which, W;              // which: the quantities this launch writes; W: doubles per vertex of the record
};

// C_D(m) of the three formulations; `method` is uniform
__device__ __forceinline__ double swe_atm_drag(double m, int method)
{
#pragma clang fp contract(off)
    if (method == SWE2D_ATM_LARGE_POND_1981) return m > 11.0 ? 1.0e-3*(0.49 + 0.065*m) : 1.2e-3;
    if (method == SWE2D_ATM_SMITH_BANKE_1975) return (0.63 + 0.066*m)/1000.;
    const double m2 = m*m, m6 = m2*m2*m2;
    const double cd = 1.e-3*(2.7/(m + 1e-3) + 0.142 + m/13.09 - 3.14807e-10*m6);
    return m > 33.0 ? 2.34e-3 : cd;
}

// grid (ceil(n_cells/256), NPC): blockIdx.y is the node, the lanes of a row of workgroups walk the cells of its plane
template <int NPC>
__global__ void __launch_bounds__(256) swe_atm_kernel(SweAtmArgs a)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x*blockDim.x + threadIdx.x;
    if (c >= a.n_cells) return;
    const int i = blockIdx.y;
    const size_t S = a.stride;
    const unsigned c8 = (unsigned)c*8u;
    const int vi = swe_ldi(swe_rsrc(a.cv + (size_t)i*S), (unsigned)c*4u, 0u);
    const unsigned r8 = (unsigned)vi*(unsigned)a.W*8u;
    const swe_rsrc_t r0 = swe_rsrc(a.s0), r1 = swe_rsrc(a.s1);
    const double al = a.alpha, om = 1.0 - al;
    if (a.which & 1) {
        const double u0 = swe_ld(r0, r8, 0u), v0 = swe_ld(r0, r8, 8u), u1 = swe_ld(r1, r8, 0u), v1 = swe_ld(r1, r8, 8u);
        const double u = om*u0 + al*u1, v = om*v0 + al*v1;
        const double m = sqrt(u*u + v*v);
        const double tau = swe_atm_drag(m, a.method)*SWE2D_ATM_RHO_AIR*m;
        swe_st(swe_rsrc(a.wind + (size_t)i*S), c8, 0u, tau*u);
        swe_st(swe_rsrc(a.wind + (size_t)(NPC + i)*S), c8, 0u, tau*v);
    }
    if (a.which & 2) {
        const unsigned po = a.W == 3 ? 16u : 0u;                          // by the record's layout: `which` is the write mask of this launch
        const double p0 = swe_ld(r0, r8, po), p1 = swe_ld(r1, r8, po);
        swe_st(swe_rsrc(a.patm + (size_t)i*S), c8, 0u, om*p0 + al*p1);
    }
}

namespace {

const char *const kAtmCapture = "atmospheric forcing calls are not allowed inside a stream capture";

// j = the largest index with times[j] <= t, clamped to 0 .. n_t - 2; alpha with the reference's RELTOL = 1e-6 of slack, clamped
bool atm_bracket(const Handle::Atm &am, double t, int *j, double *alpha)
{
#pragma clang fp contract(off)
    const std::vector<double> &tm = am.times;
    int k = (int)(std::upper_bound(tm.begin(), tm.end(), t) - tm.begin()) - 1;
    k = std::min(std::max(k, 0), am.n_t - 2);
    double al = (t - tm[k])/(tm[k + 1] - tm[k]);
    if (!(al >= -1e-6 && al <= 1.0 + 1e-6)) return false;
    *j = k;
    *alpha = al < 0.0 ? 0.0 : (al > 1.0 ? 1.0 : al);
    return true;
}

int atm_outside(Handle *h, const char *who, double t)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: time %.17g is outside the atmospheric record [%.17g, %.17g]", who, t, h->atm.times.front(),
             h->atm.times.back());
    return fail(h, SWE2D_ERR_INVALID_ARGUMENT, buf);
}

// an allocation whose failure names the bytes asked for
int atm_alloc(Handle *h, DevArray<double> &p, size_t bytes, const char *what)
{
    const hipError_t e = p.alloc(bytes/sizeof(double));
    if (e == hipSuccess) return SWE2D_OK;
    (void)hipGetLastError();
    return fail(h, SWE2D_ERR_HIP, std::string("swe2d_atm_set: ") + std::to_string(bytes) + " bytes of " + what + ": " + hipGetErrorString(e));
}

}  // namespace

int swe2d_impl::atm_launch(Handle *h, double t)
{
    const Handle::Atm &am = h->atm;
    int j = 0;
    SweAtmArgs a{};
    if (!atm_bracket(am, t, &j, &a.alpha)) return atm_outside(h, "atmospheric forcing", t);
    const size_t snap = (size_t)h->n_vertices*am.W;
    a.s0 = am.tab + (size_t)j*snap; a.s1 = a.s0 + snap;
    a.cv = h->cv;
    a.wind = h->field[SWE2D_FIELD_WIND_STRESS]; a.patm = h->field[SWE2D_FIELD_ATMOSPHERIC_PRESSURE];
    a.stride = h->stride;
    a.n_cells = h->n_cells; a.method = am.method; a.W = am.W;
    // (a field freed behind the table's back - swe2d_set_field(h, field, NULL) - is no longer written)
    a.which = am.which & ((a.wind ? 1 : 0) | (a.patm ? 2 : 0));
    if (!a.which) return SWE2D_OK;
    const dim3 grid((unsigned)grid_for(h->n_cells), (unsigned)h->npc);       // the lanes past n_cells return
    SWE_CHK_SYNC(h->stream);
    if (h->npc == 4) hipLaunchKernelGGL(swe_atm_kernel<4>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(swe_atm_kernel<3>, grid, dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

// every stage time of an advance of n_steps that is about to be enqueued lies inside the record (else nothing is enqueued)
int swe2d_impl::atm_check_advance(Handle *h, int n_steps, bool forward_euler)
{
    if (h->atm.n_t == 0) return SWE2D_OK;
    int j;
    double al;
    for (int k = 0; k < n_steps; k++)
        for (int i = forward_euler ? -1 : 0; i < (forward_euler ? 0 : 3); i++) {
            const double t = tide_stage_time(h, k, i);
            if (!atm_bracket(h->atm, t, &j, &al)) return atm_outside(h, "advance", t);
        }
    return SWE2D_OK;
}

extern "C" {

int swe2d_atm_set(swe2d_handle *hh, int32_t n_times, const double *times, const double *wind_u, const double *wind_v,
                  const double *pressure, int32_t method, int32_t which)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, kAtmCapture);
    if (which < 1 || which > 3) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: `which` must be 1 (wind), 2 (pressure) or 3");
    if (n_times < 2 || !times) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: at least two snapshot times are required");
    if (((which & 1) && (!wind_u || !wind_v)) || ((which & 2) && !pressure))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: null table of a quantity `which` names");
    if (method < SWE2D_ATM_LARGE_YEAGER_2009 || method > SWE2D_ATM_SMITH_BANKE_1975)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: unknown wind stress method");
    for (int k = 0; k < n_times; k++)
        if (!std::isfinite(times[k]) || (k > 0 && !(times[k] > times[k - 1])))
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: the times must be finite and strictly increasing");
    const size_t nv = (size_t)h->n_vertices, nt = (size_t)n_times, W = (size_t)((which & 1) ? 2 : 0) + ((which & 2) ? 1 : 0);
    // one raw buffer resource (32-bit byte offsets) spans one snapshot, one a plane of the fields, one a plane of cv
    if (nv*W*sizeof(double) >= ((size_t)1 << 32) || (size_t)h->stride*sizeof(double) >= ((size_t)1 << 32))
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_atm_set: mesh too large for the 32-bit offsets of the atmospheric kernel");
    std::vector<double> host(nt*nv*W);
    for (size_t k = 0; k < nt; k++)
        for (size_t v = 0; v < nv; v++) {
            double *r = &host[(k*nv + v)*W];
            if (which & 1) { r[0] = wind_u[k*nv + v]; r[1] = wind_v[k*nv + v]; r += 2; }
            if (which & 2) r[0] = pressure[k*nv + v];
        }
    for (double x : host) if (!std::isfinite(x)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_set: the tables must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    // build aside: the table and whatever field planes are absent; a failure leaves the handle as it was
    DevArray<double> tab, wind, patm;
    const size_t plane_bytes = (size_t)h->npc*h->stride*sizeof(double);
    int rc = atm_alloc(h, tab, host.size()*sizeof(double), "atmospheric record");
    if (!rc && (which & 1) && !h->field[SWE2D_FIELD_WIND_STRESS]) rc = atm_alloc(h, wind, 2*plane_bytes, "wind stress planes");
    if (!rc && (which & 2) && !h->field[SWE2D_FIELD_ATMOSPHERIC_PRESSURE]) rc = atm_alloc(h, patm, plane_bytes, "pressure planes");
    hipError_t e = hipSuccess;
    if (!rc) e = hipStreamSynchronize(h->stream);                         // launches that read the old table are done
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(tab, host.data(), host.size()*sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (!rc && e == hipSuccess && wind) e = hipMemsetAsync(wind, 0, 2*plane_bytes, h->stream);
    if (!rc && e == hipSuccess && patm) e = hipMemsetAsync(patm, 0, plane_bytes, h->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) {
        (void)hipGetLastError();
        rc = fail(h, SWE2D_ERR_HIP, std::string("swe2d_atm_set: ") + hipGetErrorString(e));
    }
    if (rc) return rc;
    // move in
    if (wind) h->field[SWE2D_FIELD_WIND_STRESS] = std::move(wind);
    if (patm) h->field[SWE2D_FIELD_ATMOSPHERIC_PRESSURE] = std::move(patm);
    Handle::Atm &am = h->atm;
    am.tab = std::move(tab);
    am.times.assign(times, times + nt);
    am.which = which; am.method = method; am.W = (int)W;
    am.n_t = n_times;                                                     // from here on the handle has a record (step_kernels)
    return SWE2D_OK;
}

int swe2d_atm_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, kAtmCapture);
    if (h->atm.n_t == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->atm = Handle::Atm();
    return SWE2D_OK;
}

int swe2d_atm_eval(swe2d_handle *hh, double t)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    // the time is a kernel argument: a replay of the captured launch would repeat it
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, kAtmCapture);
    if (h->atm.n_t == 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_eval: no atmospheric record (swe2d_atm_set)");
    if (!std::isfinite(t)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_eval: t must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    return atm_launch(h, t);
}

int swe2d_atm_read(swe2d_handle *hh, double *wind_nodal, double *pressure_nodal)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, kAtmCapture);
    if ((wind_nodal && !h->field[SWE2D_FIELD_WIND_STRESS]) || (pressure_nodal && !h->field[SWE2D_FIELD_ATMOSPHERIC_PRESSURE]))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_atm_read: the handle has no planes of that field");
    HIP_TRY(h, hipSetDevice(h->device));
    // through a host buffer, [component][node][stride] -> [n_cells][npc][ncomp]: not a hot path
    const size_t S = h->stride, n = (size_t)h->n_cells;
    const int npc = h->npc;
    std::vector<double> tmp((size_t)2*npc*S);
    for (int pass = 0; pass < 2; pass++) {
        double *out = pass == 0 ? wind_nodal : pressure_nodal;
        if (!out) continue;
        const int ncomp = pass == 0 ? 2 : 1;
        const double *planes = h->field[pass == 0 ? SWE2D_FIELD_WIND_STRESS : SWE2D_FIELD_ATMOSPHERIC_PRESSURE];
        HIP_TRY(h, hipMemcpyAsync(tmp.data(), planes, (size_t)ncomp*npc*S*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t c = 0; c < n; c++)
            for (int i = 0; i < npc; i++)
                for (int k = 0; k < ncomp; k++) out[(c*npc + i)*ncomp + k] = tmp[(size_t)(npc*k + i)*S + c];
    }
    return SWE2D_OK;
}

}  // extern "C"
