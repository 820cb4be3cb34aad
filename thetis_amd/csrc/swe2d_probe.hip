// swe2d_probe.hip - point probes (gauges / detectors, Function.at): the gather kernel and the swe2d_probe_* entry points.
//
// One lane per point: the lane reads its device cell and nodal weights, then for every component of the set the cell's nodal values
// from the SoA planes of buffer A (h->state[0], or a tracer's buffer A) and writes  w0*v0 + w1*v1 + w2*v2 (+ w3*v3),  left to
// right without contraction, into row `row` of the set's device buffer.  The plane pointers are taken from the handle when a
// row is enqueued, so a row appended after a launch that swapped the state buffers (swe_fuse123_kernel) reads the step result.
// The nodal values are those swe2d_get_state / swe2d_tracer_get_state return (wetting-drying: D -> eta as swe_planes_to_aos does
// it), hence a probe value has the bits of the same weighted sum computed on the host from those arrays.
#include "swe2d_handle.h"

#define SWE_PROBE_MAX_COMP 16

struct SweProbeArgs {
    const double *plane[SWE_PROBE_MAX_COMP];    // the node-0 plane of every component; node i is i*stride further
    int wd[SWE_PROBE_MAX_COMP];                 // 1: the plane holds the displaced depth D (wetting-drying), the probe gives eta
    const int *cell;                            // [n_points] device cells
    const double *weight;                       // [n_points][NPC]
    double *out;                                // [rows][n_points][width]
    const int *cv;                              // [NPC][stride] cell vertices (wetting-drying only)
    const double *vh, *valpha;                  // per-vertex bathymetry and alpha (wetting-drying only)
    size_t stride;
    int n_points, width, row;
};

template <int NPC>
__global__ void __launch_bounds__(256) swe_probe_kernel(SweProbeArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x*blockDim.x + threadIdx.x;
    if (p >= a.n_points) return;
    const size_t S = a.stride;
    const int k = swe_ldi(swe_rsrc(a.cell), (unsigned)p*4u, 0u);
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u;
    double w[NPC];
#pragma unroll
    for (int i = 0; i < NPC; i++) w[i] = swe_ld(swe_rsrc(a.weight), (unsigned)(p*NPC + i)*8u, 0u);
    const swe_rsrc_t out = swe_rsrc(a.out + (size_t)a.row*a.n_points*a.width);
    const unsigned o8 = (unsigned)p*(unsigned)a.width*8u;
    for (int c = 0; c < a.width; c++) {                   // uniform: the component table is read with scalar loads
        double v[NPC];
#pragma unroll
        for (int i = 0; i < NPC; i++) v[i] = swe_ld(swe_rsrc(a.plane[c] + (size_t)i*S), k8, 0u);
        if (a.wd[c]) {
#pragma unroll
            for (int i = 0; i < NPC; i++) {
                const int vi = swe_ldi(swe_rsrc(a.cv + (size_t)i*S), k4, 0u);
                const double al = swe_ld(swe_rsrc(a.valpha), (unsigned)vi*8u, 0u);
                const double hv = swe_ld(swe_rsrc(a.vh), (unsigned)vi*8u, 0u);
                const double e = v[i];
                v[i] = e - 0.25*al*al/e - hv;                  // swe_planes_to_aos
            }
        }
        double s = w[0]*v[0];
#pragma unroll
        for (int i = 1; i < NPC; i++) s = s + w[i]*v[i];
        swe_st(out, o8 + (unsigned)c*8u, 0u, s);
    }
}

namespace {

bool capturing(Handle *h)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool yes = h->stream && hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return yes;
}

// the handle, the set and no stream capture: 0, else the status to return
int probe_check(Handle *h, int id, Handle::Probe **out)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "probe calls are not allowed inside a stream capture");
    if (id < 0 || id >= (int)h->probes.size() || !h->probes[id].live)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "no such probe set");
    *out = &h->probes[id];
    return SWE2D_OK;
}

int launch_probe(Handle *h, const Handle::Probe &p, int row)
{
    SweProbeArgs a{};
    int c = 0;
    const size_t S = h->stride;
    for (int f : p.fields) {
        if (f == SWE2D_PROBE_UV) {
            a.plane[c++] = h->state[0];
            a.plane[c++] = h->state[0] + (size_t)h->npc*S;
        } else if (f == SWE2D_PROBE_ELEV) {
            a.wd[c] = (h->wd && h->state_holds_D) ? 1 : 0;             // as swe2d_get_state decides it
            a.plane[c++] = h->state[0] + (size_t)2*h->npc*S;
        } else {
            a.plane[c++] = h->tracers[f].buf[0];
        }
    }
    a.cell = p.cell; a.weight = p.weight; a.out = p.out;
    a.cv = h->cv; a.vh = h->vh; a.valpha = h->valpha;
    a.stride = S;
    a.n_points = p.n_points; a.width = p.width; a.row = row;
    SWE_CHK_SYNC(h->stream);
    if (h->npc == 4) hipLaunchKernelGGL(swe_probe_kernel<4>, dim3(grid_for(p.n_points)), dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(swe_probe_kernel<3>, dim3(grid_for(p.n_points)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

}  // namespace

int swe2d_probe_create(swe2d_handle *hh, int32_t n_points, const int32_t *cells, const double *weights, int32_t n_fields,
                       const int32_t *fields, int32_t capacity, int32_t *probe_id)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "probe calls are not allowed inside a stream capture");
    if (n_points <= 0 || !cells || !weights || n_fields <= 0 || !fields || capacity < 0 || !probe_id)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_create: bad argument");
    for (int i = 0; i < n_points; i++)
        if (cells[i] < 0 || cells[i] >= h->n_cells) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_create: cell out of range");
    int width = 0;
    for (int j = 0; j < n_fields; j++) {
        const int f = fields[j];
        if (f == SWE2D_PROBE_UV) width += 2;
        else if (f == SWE2D_PROBE_ELEV) width += 1;
        else if (f >= 0 && f < (int)h->tracers.size()) width += 1;
        else return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_create: unknown field");
    }
    if (width > SWE_PROBE_MAX_COMP) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_create: more than 16 components");
    const size_t row_bytes = (size_t)n_points*width*sizeof(double);
    if (((size_t)capacity + 1)*row_bytes >= (1ull << 32))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_create: the row buffer would exceed 4 GiB");
    HIP_TRY(h, hipSetDevice(h->device));
    Handle::Probe p;
    p.n_points = n_points; p.width = width; p.capacity = capacity;
    p.fields.assign(fields, fields + n_fields);
    HIP_TRY(h, p.cell.alloc(n_points));
    HIP_TRY(h, p.weight.alloc((size_t)n_points*h->npc));
    HIP_TRY(h, p.out.alloc(((size_t)capacity + 1)*n_points*width));
    HIP_TRY(h, hipMemcpyAsync(p.cell, cells, (size_t)n_points*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(p.weight, weights, (size_t)n_points*h->npc*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // the host arrays may be reused by the caller
    p.live = true;
    int id = 0;
    while (id < (int)h->probes.size() && h->probes[id].live) id++;
    if (id == (int)h->probes.size()) h->probes.push_back(std::move(p)); else h->probes[id] = std::move(p);
    *probe_id = id;
    return SWE2D_OK;
}

int swe2d_probe_width(swe2d_handle *hh, int32_t id, int32_t *n_points, int32_t *n_components, int32_t *capacity)
{
    Handle *h = H(hh);
    Handle::Probe *p = nullptr;
    if (int rc = probe_check(h, id, &p)) return rc;
    if (n_points) *n_points = p->n_points;
    if (n_components) *n_components = p->width;
    if (capacity) *capacity = p->capacity;
    return SWE2D_OK;
}

int swe2d_probe_append(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Probe *p = nullptr;
    if (int rc = probe_check(h, id, &p)) return rc;
    if (p->rows >= p->capacity) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_probe_append: the probe set is full (read it first)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = launch_probe(h, *p, p->rows)) return rc;
    p->rows++;
    return SWE2D_OK;
}

int swe2d_probe_read(swe2d_handle *hh, int32_t id, double *out, int32_t *n_rows)
{
    Handle *h = H(hh);
    Handle::Probe *p = nullptr;
    if (int rc = probe_check(h, id, &p)) return rc;
    if (!out || !n_rows) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (p->rows > 0)
        HIP_TRY(h, hipMemcpyAsync(out, p->out, (size_t)p->rows*p->n_points*p->width*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_rows = p->rows;
    p->rows = 0;
    if (int rc = capture_parity_check(h)) return rc;
    return flow_check(h);
}

int swe2d_probe_eval(swe2d_handle *hh, int32_t id, double *out)
{
    Handle *h = H(hh);
    Handle::Probe *p = nullptr;
    if (int rc = probe_check(h, id, &p)) return rc;
    if (!out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = capture_parity_check(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = launch_probe(h, *p, p->capacity)) return rc;              // the spare last row
    HIP_TRY(h, hipMemcpyAsync(out, p->out + (size_t)p->capacity*p->n_points*p->width, (size_t)p->n_points*p->width*sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return flow_check(h);
}

int swe2d_probe_destroy(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Probe *p = nullptr;
    if (int rc = probe_check(h, id, &p)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                           // rows may still be in flight
    *p = Handle::Probe();
    return SWE2D_OK;
}
