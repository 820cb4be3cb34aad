// swe2d_sections.hip - section transports: the swe2d_sections_* entry points and the kernel.
//
// A section is a list of pieces - straight segments inside one cell, cut and weighted by the host (thetis_amd/sections.py) - and
// swe_section_transport_kernel is one lane per piece: it gathers the nodal u, v, eta (and up to four tracers) of the piece's cell
// from buffer A and h through cv / vh, evaluates them at the piece's two Gauss-Legendre points with the weights handed in, and adds
//     transport  F_0 + F_1,   area  L (H_0 + H_1),   tracer t  fma(F_1, c_t1, F_0 c_t0),      F_q = H_q fma(u_q, Nx, v_q Ny)
// to the section's limb sums (swe_sum_accumulate: exact and order-independent).  The device holds no geometry of its own.  Every
// section's pieces start at a workgroup boundary (SweSectionArgs::block0, like SweFarm::block0): the wave reduction needs no section
// index per lane, padding lanes carry cell -1 and add zeros.  One launch serves all sections; it is tiny and latency-bound.
// No contraction and the fused multiply-adds written out: thetis_amd/sections.py (HostSections) restates every term bit for bit.
#include "swe2d_handle.h"

static_assert(SWE2D_SECTION_LIMBS == SWE_SUM_LIMBS, "limbs per sum mismatch");
#define SWE_SECTION_ACC (SWE2D_MAX_SECTIONS*SWE2D_SECTION_VALUES*SWE_SUM_LIMBS)
#define SWE_SECTION_ROW (SWE_SECTION_ACC + 1)                 // limb sums of every slot's values + the counter of terms that were not summed
#define SWE_SECTION_MAX_PIECES (1 << 22)

struct SweSectionArgs {
    int block0[SWE2D_MAX_SECTIONS + 1];                       // first workgroup of every slot; uniform, read with scalar loads
    const double *state;                                      // buffer A: u planes | v planes | elevation planes, [3*NPC][stride]
    const double *tracer[SWE2D_MAX_SECTION_TRACERS];          // the named tracers' buffers A, [NPC][stride]
    const int *cell;                                          // [n_lanes]
    const double *geom;                                       // [2*NPC + 3][n_lanes]
    const int *cv;                                            // [NPC][stride] cell vertices
    const double *vh;                                         // per-vertex bathymetry
    unsigned long long *row;                                  // [SWE_SECTION_ROW]
    size_t stride;
    int n_lanes, n_tracers, nonlinear;
};

// w[0] f[0] + w[1] f[1] + ... as a chain of fused multiply-adds, first term a plain product
template <int NPC>
__device__ __forceinline__ double swe_section_at(const double (&w)[NPC], const double (&f)[NPC])
{
#pragma clang fp contract(off)
    double s = w[0]*f[0];
#pragma unroll
    for (int i = 1; i < NPC; i++) s = fma(w[i], f[i], s);
    return s;
}

template <int NPC>
__global__ void __launch_bounds__(SWE_BLOCK) swe_section_transport_kernel(SweSectionArgs a)
{
#pragma clang fp contract(off)
    int s = 0;                                                // the block's section: the last slot that starts at or before it
    for (int j = 1; j < SWE2D_MAX_SECTIONS; j++)
        if ((int)blockIdx.x >= a.block0[j]) s = j;
    const int t = (int)blockIdx.x*SWE_BLOCK + (int)threadIdx.x;           // < n_lanes: the grid is n_lanes/SWE_BLOCK workgroups
    double T = 0.0, A = 0.0, C[SWE2D_MAX_SECTION_TRACERS] = {0.0, 0.0, 0.0, 0.0};
    const int k = t < a.n_lanes ? swe_ldi(swe_rsrc(a.cell), (unsigned)t*4u, 0u) : -1;
    if (k >= 0) {
        const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)a.stride*8u, S4 = (unsigned)a.stride*4u;
        const unsigned t8 = (unsigned)t*8u, L8 = (unsigned)a.n_lanes*8u;
        double w0[NPC], w1[NPC], u[NPC], v[NPC], e[NPC], h[NPC];
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            w0[i] = swe_ld(swe_rsrc(a.geom), t8, i*L8);
            w1[i] = swe_ld(swe_rsrc(a.geom), t8, (NPC + i)*L8);
            u[i] = swe_ld(swe_rsrc(a.state), k8, i*S8);
            v[i] = swe_ld(swe_rsrc(a.state + (size_t)NPC*a.stride), k8, i*S8);
            e[i] = swe_ld(swe_rsrc(a.state + (size_t)2*NPC*a.stride), k8, i*S8);
            const int vid = swe_ldi(swe_rsrc(a.cv), k4, i*S4);
            h[i] = swe_ld(swe_rsrc(a.vh), (unsigned)vid*8u, 0u);
        }
        const double Nx = swe_ld(swe_rsrc(a.geom), t8, (2*NPC)*L8), Ny = swe_ld(swe_rsrc(a.geom), t8, (2*NPC + 1)*L8);
        const double L = swe_ld(swe_rsrc(a.geom), t8, (2*NPC + 2)*L8);
        const double h0 = swe_section_at<NPC>(w0, h), h1 = swe_section_at<NPC>(w1, h);
        const double H0 = a.nonlinear ? swe_section_at<NPC>(w0, e) + h0 : h0;
        const double H1 = a.nonlinear ? swe_section_at<NPC>(w1, e) + h1 : h1;
        const double F0 = H0*fma(swe_section_at<NPC>(w0, u), Nx, swe_section_at<NPC>(w0, v)*Ny);
        const double F1 = H1*fma(swe_section_at<NPC>(w1, u), Nx, swe_section_at<NPC>(w1, v)*Ny);
        T = F0 + F1;
        A = L*(H0 + H1);
#pragma unroll
        for (int m = 0; m < SWE2D_MAX_SECTION_TRACERS; m++) {
            if (m < a.n_tracers) {                            // uniform
                double c[NPC];
#pragma unroll
                for (int i = 0; i < NPC; i++) c[i] = swe_ld(swe_rsrc(a.tracer[m]), k8, i*S8);
                C[m] = fma(F1, swe_section_at<NPC>(w1, c), F0*swe_section_at<NPC>(w0, c));
            }
        }
    }
    unsigned long long *acc = a.row + (size_t)s*SWE2D_SECTION_VALUES*SWE_SUM_LIMBS, *bad = a.row + SWE_SECTION_ACC;
    swe_sum_accumulate(T, acc, bad);
    swe_sum_accumulate(A, acc + SWE_SUM_LIMBS, bad);
#pragma unroll
    for (int m = 0; m < SWE2D_MAX_SECTION_TRACERS; m++)
        if (m < a.n_tracers) swe_sum_accumulate(C[m], acc + (size_t)(2 + m)*SWE_SUM_LIMBS, bad);
}

namespace {

int sections_rows_alloc(Handle *h, Handle::Sections &s, int capacity)
{
    if (s.rows && s.rows_cap == capacity) return SWE2D_OK;
    if (s.rows) HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, s.rows.alloc(((size_t)capacity + 1)*SWE_SECTION_ROW));
    s.rows_cap = capacity;
    s.rows_n = 0;
    return SWE2D_OK;
}

// what every call checks first; `need`: the call evaluates, so the handle must have sections and no wetting-drying
int sections_check(Handle *h, bool need)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "section calls are not allowed inside a stream capture");
    if (need && h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "section transports are not available with wetting-drying");
    if (need && h->sections.n_lanes == 0) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "the handle has no sections (swe2d_sections_set)");
    return SWE2D_OK;
}

// the one launch: the limb sums of every section of the state in buffer A, added to `row` (zeroed by the caller)
int launch_sections(Handle *h, unsigned long long *row)
{
    const Handle::Sections &s = h->sections;
    SweSectionArgs a{};
    for (int j = 0; j <= SWE2D_MAX_SECTIONS; j++) a.block0[j] = s.block0[j];
    a.state = h->state[0];
    for (int m = 0; m < s.n_tracers; m++) {
        if (s.tracer_ids[m] >= (int)h->tracers.size()) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "a section tracer no longer exists");
        a.tracer[m] = h->tracers[s.tracer_ids[m]].buf[0];     // taken when the launch is enqueued: the buffers rotate
    }
    a.cell = s.cell; a.geom = s.geom;
    a.cv = h->cv; a.vh = h->vh;
    a.row = row;
    a.stride = h->stride;
    a.n_lanes = s.n_lanes; a.n_tracers = s.n_tracers;
    a.nonlinear = h->par.use_nonlinear_equations ? 1 : 0;
    SWE_CHK_SYNC(h->stream);
    const dim3 grid((unsigned)(s.n_lanes/SWE_BLOCK));
    if (h->npc == 4) hipLaunchKernelGGL(swe_section_transport_kernel<4>, grid, dim3(SWE_BLOCK), 0, h->stream, a);
    else hipLaunchKernelGGL(swe_section_transport_kernel<3>, grid, dim3(SWE_BLOCK), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

void row_to_values(const unsigned long long *row, double *values)
{
    for (int q = 0; q < SWE2D_MAX_SECTIONS*SWE2D_SECTION_VALUES; q++) {
        int64_t limbs[SWE_SUM_LIMBS];
        for (int j = 0; j < SWE_SUM_LIMBS; j++) limbs[j] = (int64_t)row[(size_t)q*SWE_SUM_LIMBS + j];
        values[q] = swe2d_sum_limbs_to_double(limbs);
    }
}

}  // namespace

extern "C" {

int swe2d_sections_set(swe2d_handle *hh, int32_t n_sections, int32_t n_pieces, const int32_t *piece_section, const int32_t *piece_cell,
                       const double *piece_weights, const double *piece_normal, int32_t n_tracers, const int32_t *tracer_ids)
{
#pragma clang fp contract(off)
    Handle *h = H(hh);
    if (int rc = sections_check(h, false)) return rc;
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "section transports are not available with wetting-drying");
    if (n_sections < 1 || n_sections > SWE2D_MAX_SECTIONS)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: the number of sections must be in 1 .. SWE2D_MAX_SECTIONS");
    if (n_tracers < 0 || n_tracers > SWE2D_MAX_SECTION_TRACERS)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: the number of tracers must be in 0 .. SWE2D_MAX_SECTION_TRACERS");
    if (n_pieces < 1 || n_pieces > SWE_SECTION_MAX_PIECES || !piece_section || !piece_cell || !piece_weights || !piece_normal
        || (n_tracers > 0 && !tracer_ids))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: bad argument");
    for (int m = 0; m < n_tracers; m++)
        if (tracer_ids[m] < 0 || tracer_ids[m] >= (int)h->tracers.size())
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: unknown tracer id");
    const int npc = h->npc;
    int count[SWE2D_MAX_SECTIONS] = {0};
    for (int p = 0; p < n_pieces; p++) {
        if (piece_section[p] < 0 || piece_section[p] >= n_sections)
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: a piece names a section outside 0 .. n_sections-1");
        if (piece_cell[p] < 0 || piece_cell[p] >= h->n_owned)
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: a piece names a cell outside 0 .. n_owned-1");
        for (int j = 0; j < 2*npc; j++)
            if (!std::isfinite(piece_weights[(size_t)p*2*npc + j]))
                return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: the weights must be finite");
        if (!std::isfinite(piece_normal[2*(size_t)p]) || !std::isfinite(piece_normal[2*(size_t)p + 1]))
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_set: the normals must be finite");
        count[piece_section[p]]++;
    }
    // every section's pieces in the order given, padded to whole workgroups
    Handle::Sections fresh;
    int next[SWE2D_MAX_SECTIONS];
    for (int s = 0; s < SWE2D_MAX_SECTIONS; s++) {
        next[s] = fresh.block0[s]*SWE_BLOCK;
        fresh.block0[s + 1] = fresh.block0[s] + (count[s] + SWE_BLOCK - 1)/SWE_BLOCK;
    }
    const int n_lanes = fresh.block0[SWE2D_MAX_SECTIONS]*SWE_BLOCK;
    const int n_geom = 2*npc + 3;
    std::vector<int> cell((size_t)n_lanes, -1);
    std::vector<double> geom((size_t)n_geom*n_lanes, 0.0);
    for (int p = 0; p < n_pieces; p++) {
        const int t = next[piece_section[p]]++;
        cell[t] = piece_cell[p];
        for (int j = 0; j < 2*npc; j++) geom[(size_t)j*n_lanes + t] = piece_weights[(size_t)p*2*npc + j];
        const double Nx = piece_normal[2*(size_t)p], Ny = piece_normal[2*(size_t)p + 1];
        geom[(size_t)(2*npc)*n_lanes + t] = Nx;
        geom[(size_t)(2*npc + 1)*n_lanes + t] = Ny;
        geom[(size_t)(2*npc + 2)*n_lanes + t] = std::sqrt(Nx*Nx + Ny*Ny);        // len/2: two roundings and IEEE's square root
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // launches that read the old tables are done
    h->sections = Handle::Sections();                                     // (a failure below leaves the handle without sections)
    Handle::Sections &s = fresh;
    s.n_tracers = n_tracers;
    for (int m = 0; m < n_tracers; m++) s.tracer_ids[m] = tracer_ids[m];
    HIP_TRY(h, s.cell.alloc(cell.size()));
    HIP_TRY(h, s.geom.alloc(geom.size()));
    HIP_TRY(h, hipMemcpy(s.cell, cell.data(), cell.size()*sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(s.geom, geom.data(), geom.size()*sizeof(double), hipMemcpyHostToDevice));
    s.n_lanes = n_lanes;
    if (int rc = sections_rows_alloc(h, s, 0)) return rc;
    HIP_TRY(h, hipMemsetAsync(s.rows, 0, SWE_SECTION_ROW*sizeof(unsigned long long), h->stream));
    h->sections = std::move(fresh);
    return SWE2D_OK;
}

int swe2d_sections_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = sections_check(h, false)) return rc;
    if (h->sections.n_lanes == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->sections = Handle::Sections();
    return SWE2D_OK;
}

int swe2d_sections_eval_limbs(swe2d_handle *hh, int64_t *limbs, int64_t *n_unsummable)
{
    Handle *h = H(hh);
    if (int rc = sections_check(h, true)) return rc;
    if (!limbs || !n_unsummable) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = capture_parity_check(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Sections &s = h->sections;
    unsigned long long *row = s.rows + (size_t)s.rows_cap*SWE_SECTION_ROW;                  // the spare last row
    std::vector<unsigned long long> host(SWE_SECTION_ROW);
    HIP_TRY(h, hipMemsetAsync(row, 0, SWE_SECTION_ROW*sizeof(unsigned long long), h->stream));
    if (int rc = launch_sections(h, row)) return rc;
    HIP_TRY(h, hipMemcpyAsync(host.data(), row, SWE_SECTION_ROW*sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = flow_check(h)) return rc;
    for (int i = 0; i < SWE_SECTION_ACC; i++) limbs[i] = (int64_t)host[i];
    *n_unsummable = (int64_t)host[SWE_SECTION_ACC];
    return SWE2D_OK;
}

int swe2d_sections_eval(swe2d_handle *hh, double *values, int64_t *n_unsummable)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!values || !n_unsummable) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<int64_t> limbs(SWE_SECTION_ACC);
    if (int rc = swe2d_sections_eval_limbs(hh, limbs.data(), n_unsummable)) return rc;
    for (int q = 0; q < SWE2D_MAX_SECTIONS*SWE2D_SECTION_VALUES; q++) values[q] = swe2d_sum_limbs_to_double(limbs.data() + (size_t)q*SWE_SUM_LIMBS);
    return SWE2D_OK;
}

int swe2d_sections_rows_reserve(swe2d_handle *hh, int32_t capacity)
{
    Handle *h = H(hh);
    if (int rc = sections_check(h, true)) return rc;
    if (capacity < 0 || capacity > (1 << 20)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_rows_reserve: bad capacity");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = sections_rows_alloc(h, h->sections, capacity)) return rc;
    h->sections.rows_n = 0;
    HIP_TRY(h, hipMemsetAsync(h->sections.rows, 0, ((size_t)capacity + 1)*SWE_SECTION_ROW*sizeof(unsigned long long), h->stream));
    return SWE2D_OK;
}

int swe2d_sections_rows_append(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = sections_check(h, true)) return rc;
    Handle::Sections &s = h->sections;
    if (s.rows_n >= s.rows_cap)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sections_rows_append: the row store is full (reserve it / read it first)");
    HIP_TRY(h, hipSetDevice(h->device));
    // the rows were zeroed by swe2d_sections_rows_reserve / _read: the append is the one launch
    if (int rc = launch_sections(h, s.rows + (size_t)s.rows_n*SWE_SECTION_ROW)) return rc;
    s.rows_n++;
    return SWE2D_OK;
}

int swe2d_sections_rows_read(swe2d_handle *hh, double *values, int64_t *n_unsummable, int32_t *n_rows)
{
    Handle *h = H(hh);
    if (int rc = sections_check(h, false)) return rc;
    if (!n_rows) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Sections &s = h->sections;
    const int n = s.rows ? s.rows_n : 0;
    std::vector<unsigned long long> host((size_t)n*SWE_SECTION_ROW);
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(host.data(), s.rows, host.size()*sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemsetAsync(s.rows, 0, host.size()*sizeof(unsigned long long), h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_rows = n;
    s.rows_n = 0;
    if (int rc = capture_parity_check(h)) return rc;
    if (int rc = flow_check(h)) return rc;
    for (int r = 0; r < n; r++) {
        const unsigned long long *row = host.data() + (size_t)r*SWE_SECTION_ROW;
        if (values) row_to_values(row, values + (size_t)r*SWE2D_MAX_SECTIONS*SWE2D_SECTION_VALUES);
        if (n_unsummable) n_unsummable[r] = (int64_t)row[SWE_SECTION_ACC];
    }
    return SWE2D_OK;
}

}  // extern "C"
