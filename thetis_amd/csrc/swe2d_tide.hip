// swe2d_tide.hip - harmonic tidal elevation on open boundaries: the swe2d_tide_* entry points and the evaluation kernel.
//
//     eta_b(x, t) = mean(x) + sum_k A_k(x) cos(omega_k t - phi_k(x))                     (thetis/forcing.py, TidalBoundaryForcing)
//
// The table holds, for every end node of the listed boundary facets, the mean and per constituent the amplitude and the phase,
// constituent-major (amp[k][2*n_facets]): neighbouring lanes read neighbouring doubles.  swe_tide_kernel - one lane per facet node -
// writes the sum into the elevation planes of h->bc_field, the planes swe2d_set_bc_facets(h, 0, ...) writes (plane 2*facet + end
// node of the cell), and nothing else.  The time is a kernel argument: swe2d_advance enqueues one such launch in front of every
// stage launch (swe2d_plan.hip, step_swe), the step-by-step path calls swe2d_tide_eval before swe2d_solve_stage.
// The argument omega_k*t - phi and the running sum are formed left to right without contraction: the same expression in numpy
// (HarmonicTidalForcing.set_tidal_field) has the same arguments bit for bit, the two sides differ by their cosine routines only.
#include "swe2d_handle.h"

struct SweTideArgs {
    double omega[SWE2D_MAX_TIDE_CONSTITUENTS];    // uniform: read with scalar loads
    const double *mean;                         // [n_nodes]
    const double *amp, *phase;                  // [K][n_nodes]
    const int *cell, *facet;                    // [n_nodes/2] device cells and their facets
    double *planes;                             // the elevation planes of the boundary fields: [2*npc][stride]
    unsigned stride;
    int n_nodes, K;
    double t;
};

__global__ void __launch_bounds__(256) swe_tide_kernel(SweTideArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x*blockDim.x + threadIdx.x;           // facet node: facet p >> 1, its end node p & 1
    if (p >= a.n_nodes) return;
    const unsigned p8 = (unsigned)p*8u, row8 = (unsigned)a.n_nodes*8u;
    const swe_rsrc_t ra = swe_rsrc(a.amp), rp = swe_rsrc(a.phase);
    double s = swe_ld(swe_rsrc(a.mean), p8, 0u);
    for (int k = 0; k < a.K; k++) {                              // uniform trip count
        const double arg = a.omega[k]*a.t - swe_ld(rp, p8, (unsigned)k*row8);
        s = s + swe_ld(ra, p8, (unsigned)k*row8)*cos(arg);
    }
    const unsigned t4 = (unsigned)(p >> 1)*4u;
    const int c = swe_ldi(swe_rsrc(a.cell), t4, 0u), f = swe_ldi(swe_rsrc(a.facet), t4, 0u);
    // swe_bc_facet_scatter: value j of facet f of cell c -> plane 2*f + j
    swe_st(swe_rsrc(a.planes), ((unsigned)(2*f + (p & 1))*a.stride + (unsigned)c)*8u, 0u, s);
}

// the parity hook: what the elevation planes hold at the listed facet nodes
__global__ void __launch_bounds__(256) swe_tide_gather_kernel(const double *planes, unsigned stride, const int *cell, const int *facet,
                                                              int n_nodes, double *out)
{
    const int p = blockIdx.x*blockDim.x + threadIdx.x;
    if (p >= n_nodes) return;
    const unsigned t4 = (unsigned)(p >> 1)*4u;
    const int c = swe_ldi(swe_rsrc(cell), t4, 0u), f = swe_ldi(swe_rsrc(facet), t4, 0u);
    swe_st(swe_rsrc(out), (unsigned)p*8u, 0u, swe_ld(swe_rsrc(planes), ((unsigned)(2*f + (p & 1))*stride + (unsigned)c)*8u, 0u));
}


int swe2d_impl::tide_launch(Handle *h, double t)
{
    const Handle::Tide &td = h->tide;
    SweTideArgs a{};
    for (int k = 0; k < td.K; k++) a.omega[k] = td.omega[k];
    const size_t nn = 2*(size_t)td.n;
    a.mean = td.tab; a.amp = td.tab + nn; a.phase = td.tab + nn*(1 + (size_t)td.K);
    a.cell = td.list; a.facet = td.list + td.n;
    a.planes = h->bc_field[0];
    a.stride = (unsigned)h->stride;
    a.n_nodes = (int)nn; a.K = td.K;
    a.t = t;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_tide_kernel, dim3(grid_for((int)nn)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

// the time at which stage i_stage (SSPRK33: c = (0, 1, 1/2); i_stage < 0: ForwardEuler, the new time) of step `step` of the advance
// that is being enqueued is evaluated: t_k = t_base + (k_first + step)*dt, never an accumulated sum (solver2d.py: t_start + n*dt)
double swe2d_impl::tide_stage_time(const Handle *h, int step, int i_stage)
{
#pragma clang fp contract(off)
    static const double c[3] = {0.0, 1.0, 0.5};
    const double dt = h->par.dt;
    const double t_k = h->clock_t_base + (double)(h->clock_k_first + step)*dt;
    return i_stage < 0 ? t_k + dt : t_k + c[i_stage]*dt;
}

extern "C" {

int swe2d_tide_set(swe2d_handle *hh, int32_t n_facets, const int32_t *cells, const int32_t *facets, int32_t n_constituents,
                   const double *omega, const double *mean, const double *amp, const double *phase)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "tide calls are not allowed inside a stream capture");
    if (n_facets <= 0 || !cells || !facets || !omega || !mean || !amp || !phase)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: null argument or no facets");
    if (n_constituents < 1 || n_constituents > SWE2D_MAX_TIDE_CONSTITUENTS)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: the number of constituents must be in 1 .. SWE2D_MAX_TIDE_CONSTITUENTS");
    for (int t = 0; t < n_facets; t++)
        if (cells[t] < 0 || cells[t] >= h->n_cells || facets[t] < 0 || facets[t] >= h->npc)
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: cell or facet index out of range");
    // one raw buffer resource (32-bit byte offsets) spans the 2*npc elevation planes, another a row set of the table
    const size_t nn = 2*(size_t)n_facets, K = (size_t)n_constituents;
    if ((size_t)2*h->npc*h->stride*sizeof(double) >= ((size_t)1 << 32) || K*nn*sizeof(double) >= ((size_t)1 << 32))
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_tide_set: mesh or table too large for the 32-bit offsets of the tide kernel");
    for (size_t i = 0; i < nn; i++) if (!std::isfinite(mean[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: the table must be finite");
    for (size_t i = 0; i < K*nn; i++)
        if (!std::isfinite(amp[i]) || !std::isfinite(phase[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: the table must be finite");
    for (size_t k = 0; k < K; k++) if (!std::isfinite(omega[k])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_set: the table must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // launches that read the old table are done
    h->tide = Handle::Tide();                                                      // (the clock is the handle's: a new table keeps it)
    Handle::Tide &td = h->tide;
    if (!h->bc_field[0]) {                                                // as swe2d_set_bc_facets
        const size_t bytes = (size_t)2*h->npc*h->stride*sizeof(double);
        HIP_TRY(h, h->bc_field[0].alloc(bytes/sizeof(double)));
        HIP_TRY(h, hipMemsetAsync(h->bc_field[0], 0, bytes, h->stream));
    }
    HIP_TRY(h, td.tab.alloc((1 + 2*K)*nn));
    HIP_TRY(h, td.list.alloc(nn));
    HIP_TRY(h, td.out.alloc(nn));
    HIP_TRY(h, hipMemcpyAsync(td.tab, mean, nn*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(td.tab + nn, amp, K*nn*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(td.tab + nn*(1 + K), phase, K*nn*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(td.list, cells, (size_t)n_facets*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(td.list + n_facets, facets, (size_t)n_facets*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // the host arrays may be reused by the caller
    for (size_t k = 0; k < K; k++) td.omega[k] = omega[k];
    td.K = n_constituents;
    td.n = n_facets;                                                      // from here on the handle has a tide (step_kernels)
    return SWE2D_OK;
}

int swe2d_tide_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "tide calls are not allowed inside a stream capture");
    if (h->tide.n == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->tide = Handle::Tide();
    return SWE2D_OK;
}

int swe2d_tide_clock(swe2d_handle *hh, double t_base, int64_t k_first)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(t_base) || k_first < 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_clock: t_base must be finite and k_first >= 0");
    h->clock_t_base = t_base;
    h->clock_k_first = (long long)k_first;
    return SWE2D_OK;
}

int swe2d_tide_eval(swe2d_handle *hh, double t)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    // the time is a kernel argument: a replay of the captured launch would repeat it
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "tide calls are not allowed inside a stream capture");
    if (h->tide.n == 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_eval: no tide table (swe2d_tide_set)");
    if (!std::isfinite(t)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_eval: t must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    return tide_launch(h, t);
}

int swe2d_tide_read(swe2d_handle *hh, double *out)
{
    Handle *h = H(hh);
    if (!h || !out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "tide calls are not allowed inside a stream capture");
    if (h->tide.n == 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_tide_read: no tide table (swe2d_tide_set)");
    HIP_TRY(h, hipSetDevice(h->device));
    const Handle::Tide &td = h->tide;
    const int nn = 2*td.n;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_tide_gather_kernel, dim3(grid_for(nn)), dim3(256), 0, h->stream, h->bc_field[0], (unsigned)h->stride, td.list,
                       td.list + td.n, nn, td.out);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, td.out, (size_t)nn*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

}  // extern "C"
