// swe2d_stats.hip - running statistics of whole fields over every sampled step: the swe2d_stats_* entry points and the kernel.
//
// A statistics set holds 8 + 2K accumulator planes per DG node, laid out like the state: [accumulator][node][stride].  One sample
// takes the node's values e, u, v as swe2d_get_state returns them (wetting-drying: D -> eta as swe_planes_to_aos does it) and updates,
// left to right without contraction,
//
//     q = u*u + v*v            s = sqrt(q)
//     e_min = e < e_min ? e : e_min        e_max = e > e_max ? e : e_max        q_max = q > q_max ? q : q_max
//     e_sum += e    u_sum += u    v_sum += v    s_sum += s    s3_sum += q*s
//     C_k += e*wc_k        S_k += e*ws_k            (k < K; wc_k = cos(omega_k t), ws_k = sin(omega_k t), formed by the CALLER)
//
// The weights depend on time only: they travel in the kernel arguments and are read at uniform addresses in a loop of uniform trip
// count (as swe_tide_kernel reads omega), so the device evaluates no transcendental and everything but s_sum / s3_sum (the device's
// sqrt) has the bits of the same expressions in numpy.  swe_stats_kernel - one lane per node value, the node uniform per workgroup -
// is pure streaming: per node and sample it reads 24 B and read-modify-writes 16*(8 + 2K) B; no LDS, no atomics, every accumulator
// has exactly one writer.  The state plane pointers are taken from the handle when the launch is enqueued, so an append after a
// launch that swapped the state buffers (swe_fuse123_kernel) reads the step result, as a probe row does.
#include "swe2d_handle.h"

#define SWE_STATS_FIXED 8                       // e_min, e_max, q_max, e_sum, u_sum, v_sum, s_sum, s3_sum
#define SWE_STATS_READ_BYTES ((size_t)256 << 20)    // swe2d_stats_read: the host buffer of one device-to-host copy

struct SweStatsArgs {
    double w[2*SWE2D_MAX_TIDE_CONSTITUENTS];    // wc_0, ws_0, wc_1, ...: uniform, read with scalar loads
    const double *state;                        // buffer A: u planes | v planes | elevation planes, [3*NPC][stride]
    double *acc;                                // [8 + 2K][NPC][stride]
    const int *cv;                              // [NPC][stride] cell vertices (wetting-drying only)
    const double *vh, *valpha;                  // per-vertex bathymetry and alpha (wetting-drying only)
    size_t stride;
    int n_cells, K, wd;                         // wd = 1: the elevation planes hold the displaced depth D
};

// grid (ceil(n_cells/256), NPC): blockIdx.y is the node, the lanes of a row of workgroups walk the cells of its plane
template <int NPC>
__global__ void __launch_bounds__(256) swe_stats_kernel(SweStatsArgs a)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x*blockDim.x + threadIdx.x;
    if (c >= a.n_cells) return;
    const int i = blockIdx.y;
    const size_t S = a.stride;
    const unsigned c8 = (unsigned)c*8u;
    const double u = swe_ld(swe_rsrc(a.state + (size_t)i*S), c8, 0u);
    const double v = swe_ld(swe_rsrc(a.state + (size_t)(NPC + i)*S), c8, 0u);
    double e = swe_ld(swe_rsrc(a.state + (size_t)(2*NPC + i)*S), c8, 0u);
    if (a.wd) {
        const int vi = swe_ldi(swe_rsrc(a.cv + (size_t)i*S), (unsigned)c*4u, 0u);
        const double al = swe_ld(swe_rsrc(a.valpha), (unsigned)vi*8u, 0u);
        const double hv = swe_ld(swe_rsrc(a.vh), (unsigned)vi*8u, 0u);
        e = e - 0.25*al*al/e - hv;                                 // swe_planes_to_aos
    }
    const size_t P = (size_t)NPC*S;                                // one accumulator: NPC planes
    double *const node = a.acc + (size_t)i*S;                      // this node's plane of accumulator 0
    double x[SWE_STATS_FIXED];
#pragma unroll
    for (int j = 0; j < SWE_STATS_FIXED; j++) x[j] = swe_ld(swe_rsrc(node + (size_t)j*P), c8, 0u);
    const double q = u*u + v*v;
    const double s = sqrt(q);
    x[0] = e < x[0] ? e : x[0];
    x[1] = e > x[1] ? e : x[1];
    x[2] = q > x[2] ? q : x[2];
    x[3] = x[3] + e;
    x[4] = x[4] + u;
    x[5] = x[5] + v;
    x[6] = x[6] + s;
    x[7] = x[7] + q*s;
#pragma unroll
    for (int j = 0; j < SWE_STATS_FIXED; j++) swe_st(swe_rsrc(node + (size_t)j*P), c8, 0u, x[j]);
#pragma unroll 4
    for (int k = 0; k < a.K; k++) {                                // uniform trip count, uniform weights
        const swe_rsrc_t rc = swe_rsrc(node + (size_t)(SWE_STATS_FIXED + 2*k)*P), rs = swe_rsrc(node + (size_t)(SWE_STATS_FIXED + 2*k + 1)*P);
        const double ck = swe_ld(rc, c8, 0u), sk = swe_ld(rs, c8, 0u);
        swe_st(rc, c8, 0u, ck + e*a.w[2*k]);
        swe_st(rs, c8, 0u, sk + e*a.w[2*k + 1]);
    }
}

// the accumulators of an empty set: e_min = +inf, e_max = q_max = -inf, the sums 0 (the padding of the planes included)
__global__ void __launch_bounds__(256) swe_stats_fill_kernel(double *acc, size_t plane_set, size_t total)
{
    const size_t g = (size_t)blockIdx.x*blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t j = g/plane_set;
    acc[g] = j == 0 ? INFINITY : (j <= 2 ? -INFINITY : 0.0);
}

namespace {

int stats_check(Handle *h, int id, Handle::Stats **out)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "statistics calls are not allowed inside a stream capture");
    if (id < 0 || id >= (int)h->stats.size() || !h->stats[id].live)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "no such statistics set");
    *out = &h->stats[id];
    return SWE2D_OK;
}

int stats_fill(Handle *h, const Handle::Stats &s)
{
    const size_t plane_set = (size_t)h->npc*h->stride, total = (size_t)(SWE_STATS_FIXED + 2*s.K)*plane_set;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_stats_fill_kernel, dim3((unsigned)((total + 255)/256)), dim3(256), 0, h->stream, s.acc, plane_set, total);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

}  // namespace

int swe2d_stats_create(swe2d_handle *hh, int32_t n_constituents, int32_t *stats_id)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "statistics calls are not allowed inside a stream capture");
    if (!stats_id) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_stats_create: null argument");
    if (n_constituents < 0 || n_constituents > SWE2D_MAX_TIDE_CONSTITUENTS)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_stats_create: the number of constituents must be in 0 .. SWE2D_MAX_TIDE_CONSTITUENTS");
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Stats s;
    s.K = n_constituents;
    const size_t bytes = (size_t)(SWE_STATS_FIXED + 2*s.K)*h->npc*h->stride*sizeof(double);
    HIP_TRY(h, s.acc.alloc(bytes/sizeof(double)));
    if (int rc = stats_fill(h, s)) return rc;
    s.live = true;
    int id = 0;
    while (id < (int)h->stats.size() && h->stats[id].live) id++;
    if (id == (int)h->stats.size()) h->stats.push_back(std::move(s)); else h->stats[id] = std::move(s);
    *stats_id = id;
    return SWE2D_OK;
}

int swe2d_stats_append(swe2d_handle *hh, int32_t id, const double *weights)
{
    Handle *h = H(hh);
    Handle::Stats *s = nullptr;
    if (int rc = stats_check(h, id, &s)) return rc;
    if (s->K > 0 && !weights) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_stats_append: a set with constituents needs weights");
    HIP_TRY(h, hipSetDevice(h->device));
    SweStatsArgs a{};
    for (int k = 0; k < 2*s->K; k++) a.w[k] = weights[k];
    a.state = h->state[0];
    a.acc = s->acc;
    a.cv = h->cv; a.vh = h->vh; a.valpha = h->valpha;
    a.stride = h->stride;
    a.n_cells = h->n_cells; a.K = s->K;
    a.wd = (h->wd && h->state_holds_D) ? 1 : 0;                            // as swe2d_get_state decides it
    const dim3 grid((unsigned)grid_for(h->n_cells), (unsigned)h->npc);       // the lanes past n_cells return
    SWE_CHK_SYNC(h->stream);
    if (h->npc == 4) hipLaunchKernelGGL(swe_stats_kernel<4>, grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(swe_stats_kernel<3>, grid, dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    s->n_samples++;
    return SWE2D_OK;
}

int swe2d_stats_read(swe2d_handle *hh, int32_t id, double *out, int64_t *n_samples)
{
    Handle *h = H(hh);
    Handle::Stats *s = nullptr;
    if (int rc = stats_check(h, id, &s)) return rc;
    if (!out || !n_samples) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    // through a host buffer, [node][stride] -> [n_cells][npc]: the whole set in one copy where it fits SWE_STATS_READ_BYTES of
    // host memory, else as many whole accumulators per copy as do (at least one) - not a hot path
    const size_t S = h->stride, n = (size_t)h->n_cells;
    const int npc = h->npc, n_acc = SWE_STATS_FIXED + 2*s->K;
    const size_t P = (size_t)npc*S;
    const int per_copy = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_acc, SWE_STATS_READ_BYTES/(P*sizeof(double))));
    std::vector<double> tmp((size_t)per_copy*P);
    for (int j0 = 0; j0 < n_acc; j0 += per_copy) {
        const int nj = std::min(per_copy, n_acc - j0);
        HIP_TRY(h, hipMemcpyAsync(tmp.data(), s->acc + (size_t)j0*P, (size_t)nj*P*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int j = 0; j < nj; j++) {
            double *o = out + (size_t)(j0 + j)*n*npc;
            const double *t = tmp.data() + (size_t)j*P;
            for (int i = 0; i < npc; i++)
                for (size_t c = 0; c < n; c++) o[c*npc + i] = t[(size_t)i*S + c];
        }
    }
    *n_samples = (int64_t)s->n_samples;
    if (int rc = capture_parity_check(h)) return rc;
    return flow_check(h);
}

int swe2d_stats_reset(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Stats *s = nullptr;
    if (int rc = stats_check(h, id, &s)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = stats_fill(h, *s)) return rc;
    s->n_samples = 0;
    return SWE2D_OK;
}

int swe2d_stats_destroy(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Stats *s = nullptr;
    if (int rc = stats_check(h, id, &s)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                           // samples may still be in flight
    *s = Handle::Stats();
    return SWE2D_OK;
}
