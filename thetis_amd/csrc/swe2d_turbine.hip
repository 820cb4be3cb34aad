// swe2d_turbine.hip - tidal turbine farms: the swe2d_turbine_* entry points and the power kernel.
//
// The drag term itself is part of the stage kernels (swe2d_kernels.h: swe_farm_terms / swe_farm_drag_quad, from the table this unit
// uploads).  Here: per farm the nodal density planes and the compacted list of the OWNED cells in which the density is not zero, and
// swe_turbine_power_kernel - one lane per entry of a farm's cell list, the farm's power integrand
//     0.5 rho0 A_T C_P(u3^(1/3)) u3 d,   u3 = |u|^3 / alpha^3,   alpha with the static bathymetry    (turbines.py:85-93, :233, :252)
// integrated over the lane's cell with the rule of the drag term and added to the farm's limb sums (swe_sum_accumulate: exact and
// order-independent, so one handle on the whole mesh and N partitions give the same six integers).  A block works on one farm only
// (SweFarm::block0): the wave reduction needs no farm index per lane.
#include "swe2d_handle.h"

#define SWE_FARM_ROW (SWE_MAX_FARMS*SWE_SUM_LIMBS + 1)       // limb sums of every farm slot + the counter of terms that were not summed

// the power integrand at a point: speed components, static depth, density
__device__ __forceinline__ double swe_farm_power_pt(const SweFarm &F, double uq, double vq, double hq, double dq)
{
#pragma clang fp contract(off)
    const double umag = swe_sqrt(fma(uq, uq, vq*vq));
    double u3 = umag*umag*umag;
    if (F.upwind) {                                           // uniform
        const double al = swe_farm_alpha(F, swe_farm_thrust_area(F, umag), 1.0/hq);
        u3 = u3/(al*al*al);
    }
    const double cp = F.n_table > 0 ? swe_farm_table(F.speeds, F.power, F.rdx, F.n_table, cbrt(u3)) : F.power_const;
    return F.half_rho_area*cp*u3*dq;
}

template <int NPC>
__global__ void __launch_bounds__(SWE_BLOCK) swe_turbine_power_kernel(const SweFarmTable *ft, const double *planes, size_t stride, const int *cv,
                                                                      const double *vx, const double *vy, const double *vh, int affine,
                                                                      unsigned long long *row)
{
#pragma clang fp contract(off)
    int m = 0;                                                // the block's farm: the last live one that starts at or before it
    for (int j = 0; j < SWE_MAX_FARMS; j++)
        if (ft->live[j] && ft->f[j].n_list > 0 && (int)blockIdx.x >= ft->f[j].block0) m = j;
    const SweFarm &F = ft->f[m];
    const int t = ((int)blockIdx.x - F.block0)*SWE_BLOCK + (int)threadIdx.x;
    double P = 0.0;
    if (t < F.n_list) {
        const int k = swe_ldi(swe_rsrc(F.cells), (unsigned)t*4u, 0u);
        const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)stride*8u, S4 = (unsigned)stride*4u;
        double u[NPC], v[NPC], d[NPC], px[NPC], py[NPC], h[NPC];
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            u[i] = swe_ld(swe_rsrc(planes), k8, i*S8);
            v[i] = swe_ld(swe_rsrc(planes + (size_t)NPC*stride), k8, i*S8);
            d[i] = swe_ld(swe_rsrc(F.density), k8, i*S8);
            const int vid = swe_ldi(swe_rsrc(cv), k4, i*S4);
            px[i] = swe_ld(swe_rsrc(vx), (unsigned)vid*8u, 0u);
            py[i] = swe_ld(swe_rsrc(vy), (unsigned)vid*8u, 0u);
            h[i] = swe_ld(swe_rsrc(vh), (unsigned)vid*8u, 0u);
        }
        if constexpr (NPC == 3) {
            const double A = 0.5*((px[1] - px[0])*(py[2] - py[0]) - (px[2] - px[0])*(py[1] - py[0]));
            const double a1 = 0.445948490915965, b1 = 0.108103018168070, w1 = 0.223381589678011;
            const double a2 = 0.091576213509771, b2 = 0.816847572980459, w2 = 0.109951743655322;
            const double us = u[0] + u[1] + u[2], vs = v[0] + v[1] + v[2], hs = h[0] + h[1] + h[2], ds = d[0] + d[1] + d[2];
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const double aa = o ? a2 : a1, dd = o ? b2 - a2 : b1 - a1, wA = (o ? w2 : w1)*A;
#pragma unroll
                for (int i = 0; i < 3; i++)
                    P += wA*swe_farm_power_pt(F, fma(dd, u[i], aa*us), fma(dd, v[i], aa*vs), fma(dd, h[i], aa*hs), fma(dd, d[i], aa*ds));
            }
        } else {
            // det J = d0 + d1 xi + d2 zeta (swe_quad_stage_cell), 2 x 2 Gauss points
            const double ax = px[1] - px[0], ay = py[1] - py[0], bx = px[3] - px[0], by = py[3] - py[0];
            const double cx = px[0] - px[1] + px[2] - px[3], cy = py[0] - py[1] + py[2] - py[3];
            const double d0 = ax*by - ay*bx;
            const double d1 = affine ? 0.0 : ax*cy - ay*cx, d2 = affine ? 0.0 : cx*by - cy*bx;
#pragma unroll 1
            for (int q = 0; q < 4; q++) {
                const double xi = (q & 2) ? SWE_XI1 : SWE_XI0, ze = (q & 1) ? SWE_XI1 : SWE_XI0;
                const double phi[4] = {(1.0 - xi)*(1.0 - ze), xi*(1.0 - ze), xi*ze, (1.0 - xi)*ze};
                double uq = 0.0, vq = 0.0, hq = 0.0, dq = 0.0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uq = fma(phi[i], u[i], uq);
                    vq = fma(phi[i], v[i], vq);
                    hq = fma(phi[i], h[i], hq);
                    dq = fma(phi[i], d[i], dq);
                }
                P += 0.25*(d0 + d1*xi + d2*ze)*swe_farm_power_pt(F, uq, vq, hq, dq);
            }
        }
    }
    swe_sum_accumulate(P, row + (size_t)m*SWE_SUM_LIMBS, row + SWE_MAX_FARMS*SWE_SUM_LIMBS);
}

bool swe2d_impl::farm_capturing(Handle *h)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool yes = h->stream && hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return yes;
}

// the device's copy of the farms' constants, rebuilt after every change (the stream is idle: the callers synchronise first)
// A discrete slot has its constants in the table but is not live in it: the stage kernels and swe_turbine_power_kernel pass it by,
// the passes of swe2d_dfarm.hip read f[m].
int swe2d_impl::farm_upload_table(Handle *h)
{
    SweFarmTable t{};
    int blocks = 0;
    h->n_farms = h->n_cfarms = 0;
    for (int m = 0; m < SWE2D_MAX_FARMS; m++) {
        const Handle::Farm &f = h->farms[m];
        if (!f.live) continue;
        h->n_farms++;
        if (!f.discrete) h->n_cfarms++;
        const swe2d_turbine_params &p = f.par;
        SweFarm &d = t.f[m];
        t.live[m] = f.discrete ? 0 : 1;
        d.thrust_area_const = p.thrust_area_const;
        d.support_area = p.support_area;
        d.half_rho_area = 0.5*p.rho0*p.rotor_area;
        d.rdproj = 1.0/p.projected_diameter;
        d.power_const = p.power_const;
        d.rotor_area = p.rotor_area;
        d.upwind = p.upwind_correction ? 1 : 0;
        d.n_table = p.n_table;
        for (int j = 0; j < p.n_table; j++) { d.speeds[j] = p.speeds[j]; d.thrust[j] = p.thrust[j]; d.power[j] = p.power[j]; }
        for (int j = 0; j + 1 < p.n_table; j++) d.rdx[j] = 1.0/(p.speeds[j + 1] - p.speeds[j]);
        d.density = f.density;
        d.cells = f.cells;
        d.n_list = f.n_list;
        d.block0 = blocks;
        if (!f.discrete) blocks += (f.n_list + SWE_BLOCK - 1)/SWE_BLOCK;
    }
    h->farm_blocks = blocks;
    HIP_TRY(h, h->farm_table.ensure(1));
    HIP_TRY(h, hipMemcpy(h->farm_table, &t, sizeof(t), hipMemcpyHostToDevice));
    return SWE2D_OK;
}

int swe2d_impl::farm_rows_alloc(Handle *h, int capacity)
{
    if (h->farm_rows && h->farm_rows_cap == capacity) return SWE2D_OK;
    if (h->farm_rows) HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, h->farm_rows.alloc(((size_t)capacity + 1)*SWE_FARM_ROW));
    h->farm_rows_cap = capacity;
    h->farm_rows_n = 0;
    return SWE2D_OK;
}

namespace {

// one launch (and one per discrete farm): the limb sums of every farm's power of the state in buffer A, added to `row` (zeroed by
// the caller)
int launch_power(Handle *h, unsigned long long *row)
{
    if (h->n_farms > h->n_cfarms) { if (int rc = dfarm_launch_power(h, row)) return rc; }
    if (h->farm_blocks == 0) return SWE2D_OK;
    SWE_CHK_SYNC(h->stream);
    if (h->npc == 4)
        hipLaunchKernelGGL(swe_turbine_power_kernel<4>, dim3(h->farm_blocks), dim3(SWE_BLOCK), 0, h->stream, h->farm_table, h->state[0],
                           h->stride, h->cv, h->vx, h->vy, h->vh, h->affine ? 1 : 0, row);
    else
        hipLaunchKernelGGL(swe_turbine_power_kernel<3>, dim3(h->farm_blocks), dim3(SWE_BLOCK), 0, h->stream, h->farm_table, h->state[0],
                           h->stride, h->cv, h->vx, h->vy, h->vh, 1, row);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

}  // namespace

extern "C" {

int swe2d_turbine_farm_set(swe2d_handle *hh, int32_t farm, const swe2d_turbine_params *p, const double *density_nodal)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (farm < 0 || farm >= SWE2D_MAX_FARMS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: farm must be in 0 .. SWE2D_MAX_FARMS-1");
    if (!p || !density_nodal) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: null argument");
    if (p->n_table < 0 || p->n_table == 1 || p->n_table > SWE2D_MAX_THRUST_TABLE)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: n_table must be 0 or 2 .. SWE2D_MAX_THRUST_TABLE");
    for (int j = 0; j + 1 < p->n_table; j++)
        if (!(p->speeds[j + 1] > p->speeds[j])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: thrust speeds must increase strictly");
    if (!(p->projected_diameter > 0.0) || !(p->rotor_area > 0.0))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: diameters must be positive");
    const size_t n = (size_t)h->n_cells*h->npc;
    std::vector<int> list;
    for (int k = 0; k < h->n_cells; k++) {
        bool any = false;
        for (int i = 0; i < h->npc; i++) {
            const double d = density_nodal[(size_t)k*h->npc + i];
            if (!(d >= 0.0) || !std::isfinite(d)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_set: the turbine density must be finite and >= 0");
            any = any || d != 0.0;
        }
        if (any && k < h->n_owned) list.push_back(k);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // launches that read the old table / density are done
    Handle::Farm &f = h->farms[farm];
    if (f.discrete) f = Handle::Farm();                                   // the slot changes its kind
    const size_t plane_bytes = (size_t)h->npc*h->stride*sizeof(double);
    if (!f.density) {
        HIP_TRY(h, f.density.alloc(plane_bytes/sizeof(double)));
        HIP_TRY(h, hipMemsetAsync(f.density, 0, plane_bytes, h->stream));
    }
    f.cells.reset();
    f.n_list = (int)list.size();
    if (f.n_list) {
        HIP_TRY(h, f.cells.alloc(list.size()));
        HIP_TRY(h, hipMemcpyAsync(f.cells, list.data(), list.size()*sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipMemcpyAsync(h->stage_uv, density_nodal, n*sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(swe_nodal_to_planes, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, h->stage_uv, f.density, h->stride,
                       h->n_cells, 1, h->npc);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // the host arrays may be reused by the caller
    f.par = *p;
    f.live = true;
    if (!h->farm_rows) { if (int rc = farm_rows_alloc(h, 0)) return rc; }
    return farm_upload_table(h);
}

int swe2d_turbine_farm_clear(swe2d_handle *hh, int32_t farm)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (farm < 0 || farm >= SWE2D_MAX_FARMS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_farm_clear: farm must be in 0 .. SWE2D_MAX_FARMS-1");
    if (!h->farms[farm].live) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->farms[farm] = Handle::Farm();
    return farm_upload_table(h);
}

int swe2d_turbine_power_limbs(swe2d_handle *hh, int64_t limbs[SWE2D_MAX_FARMS*6])
{
    Handle *h = H(hh);
    if (!h || !limbs) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (int rc = capture_parity_check(h)) return rc;
    for (int i = 0; i < SWE2D_MAX_FARMS*SWE_SUM_LIMBS; i++) limbs[i] = 0;
    if (h->n_farms == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long *row = h->farm_rows + (size_t)h->farm_rows_cap*SWE_FARM_ROW;          // the spare last row
    unsigned long long host[SWE_FARM_ROW];
    HIP_TRY(h, hipMemsetAsync(row, 0, sizeof(host), h->stream));
    if (int rc = launch_power(h, row)) return rc;
    HIP_TRY(h, hipMemcpyAsync(host, row, sizeof(host), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = flow_check(h)) return rc;
    if (host[SWE_MAX_FARMS*SWE_SUM_LIMBS] != 0) return fail(h, SWE2D_ERR_NOT_FINITE, "turbine power is not finite");
    for (int i = 0; i < SWE2D_MAX_FARMS*SWE_SUM_LIMBS; i++) limbs[i] = (int64_t)host[i];
    return SWE2D_OK;
}

int swe2d_turbine_power(swe2d_handle *hh, double out[SWE2D_MAX_FARMS])
{
    Handle *h = H(hh);
    if (!h || !out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    int64_t limbs[SWE2D_MAX_FARMS*SWE_SUM_LIMBS];
    if (int rc = swe2d_turbine_power_limbs(hh, limbs)) return rc;
    for (int m = 0; m < SWE2D_MAX_FARMS; m++) out[m] = swe2d_sum_limbs_to_double(limbs + SWE_SUM_LIMBS*m);
    return SWE2D_OK;
}

int swe2d_turbine_rows_reserve(swe2d_handle *hh, int32_t capacity)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (capacity < 0 || capacity > (1 << 22)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_rows_reserve: bad capacity");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = farm_rows_alloc(h, capacity)) return rc;
    h->farm_rows_n = 0;
    HIP_TRY(h, hipMemsetAsync(h->farm_rows, 0, ((size_t)capacity + 1)*SWE_FARM_ROW*sizeof(unsigned long long), h->stream));
    return SWE2D_OK;
}

int swe2d_turbine_rows_append(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (!h->farm_rows || h->farm_rows_n >= h->farm_rows_cap)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_turbine_rows_append: the row store is full (reserve it / read it first)");
    HIP_TRY(h, hipSetDevice(h->device));
    // the rows were zeroed by swe2d_turbine_rows_reserve / _read: the append is the one launch
    if (int rc = launch_power(h, h->farm_rows + (size_t)h->farm_rows_n*SWE_FARM_ROW)) return rc;
    h->farm_rows_n++;
    return SWE2D_OK;
}

int swe2d_turbine_rows_read(swe2d_handle *hh, double *out, int32_t *n_rows)
{
    Handle *h = H(hh);
    if (!h || !out || !n_rows) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    HIP_TRY(h, hipSetDevice(h->device));
    const int n = h->farm_rows_n;
    std::vector<unsigned long long> host((size_t)n*SWE_FARM_ROW);
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(host.data(), h->farm_rows, host.size()*sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->farm_rows, 0, host.size()*sizeof(unsigned long long), h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_rows = n;
    h->farm_rows_n = 0;
    if (int rc = capture_parity_check(h)) return rc;
    if (int rc = flow_check(h)) return rc;
    for (int r = 0; r < n; r++) {
        const unsigned long long *row = host.data() + (size_t)r*SWE_FARM_ROW;
        if (row[SWE_MAX_FARMS*SWE_SUM_LIMBS] != 0) return fail(h, SWE2D_ERR_NOT_FINITE, "turbine power is not finite");
        for (int m = 0; m < SWE2D_MAX_FARMS; m++) {
            int64_t limbs[SWE_SUM_LIMBS];
            for (int j = 0; j < SWE_SUM_LIMBS; j++) limbs[j] = (int64_t)row[m*SWE_SUM_LIMBS + j];
            out[(size_t)r*SWE2D_MAX_FARMS + m] = swe2d_sum_limbs_to_double(limbs);
        }
    }
    return SWE2D_OK;
}

}  // extern "C"
