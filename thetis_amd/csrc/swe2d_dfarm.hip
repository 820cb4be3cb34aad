// swe2d_dfarm.hip - discrete tidal turbine farms: the swe2d_dfarm_* entry points and their three kernels.
//
// A discrete farm is a set of turbines at coordinates, each a bump density (thetis/turbines.py:174-210)
//     d(x) = sum_t psi((x - x_t)/r) psi((y - y_t)/r) / (r^2 1.45661),   psi(s) = |s| < 1 ? exp(1 - 1/(1 - s^2)) : 0,   r = D_proj/2.
// The integrand is not polynomial: the farm brings a rule of its own (up to SWE2D_MAX_FARM_QUAD points; degree 10 by default, against
// the 6 / 4 points of the stage kernels), and it touches the few cells around its turbines.  So the term is not part of the stage
// kernels but a pass over a compact cell list after each stage launch, as the SIPG viscosity:
//     U_out[uv] += beta*dt*M^-1 R_farm(U_in),   R_farm,i = - int c_t(|u|, H) d |u| u phi_i / H dx.
//   swe_dfarm_density_kernel  set-up: one lane per (listed cell, point), the bump sum over the cell's candidate turbines into a table
//                             [n_q][n_list] - the passes below read a column per point, coalesced, and no exp
//   swe_dfarm_drag_kernel     one lane per listed cell: the rule's points in a loop (phi and w at uniform addresses of the kernel
//                             arguments), swe_farm_drag_pt of the stage kernels per point, the cell's mass inverse, one writer per node
//   swe_dfarm_power_kernel    the farm's power into its slot of a power row (limb sums, as swe_turbine_power_kernel)
//   swe_dfarm_turbine_kernel  one wave per turbine over the turbine's cells, the turbine's own bump evaluated on the fly
// The farm's constants are its entry of the SweFarmTable (swe2d_turbine.hip: farm_upload_table), which is not live there.
#include "swe2d_handle.h"

#define SWE_DFARM_NORM 1.45661                              // int of psi(x) psi(y) over the square, as the reference rounds it

// the rule: kernel arguments, read with scalar loads (the point index is uniform)
struct SweDfarmRule {
    double phi[SWE2D_MAX_FARM_QUAD*4];                       // [n_q][NPC]
    double w[SWE2D_MAX_FARM_QUAD];
    int n_q;
};

struct SweDfarmArgs {
    const SweFarm *F;                                        // the farm's constants
    const double *in;                                        // state planes the term is evaluated on
    double *out;                                             // state planes whose velocity takes the update (drag pass)
    unsigned stride;
    const int *cells;                                        // [n_list]
    const double *dtab;                                      // [n_q][n_list]
    int n_list;
    const int *cv;
    const double *vx, *vy, *vh;
    int cell_begin, cell_end;                                // the stage launch's range: listed cells outside it sit the pass out
    int nonlin;                                              // H = h + eta (else h), as the stage kernels form it
    double sdt;                                              // beta*dt
    unsigned long long *row;                                 // power pass: the farm's limbs, then the row's counter of unsummed terms
    unsigned long long *bad;
};

__device__ __forceinline__ double swe_dfarm_psi(double s)
{
#pragma clang fp contract(off)
    return fabs(s) < 1.0 ? exp(1.0 - 1.0/(1.0 - s*s)) : 0.0;
}

// the point of the rule in the cell: sum_i phi_i p_i, left to right (affine on triangles and parallelograms, bilinear otherwise)
template <int NPC>
__device__ __forceinline__ double swe_dfarm_point(const double *phi, const double p[NPC])
{
#pragma clang fp contract(off)
    double x = phi[0]*p[0];
#pragma unroll
    for (int i = 1; i < NPC; i++) x = x + phi[i]*p[i];
    return x;
}

template <int NPC>
__global__ void __launch_bounds__(256) swe_dfarm_density_kernel(const SweDfarmRule R, const int *cells, int n_list, unsigned stride,
                                                                const int *cv, const double *vx, const double *vy, const int *c_off,
                                                                const int *c_idx, const double *txy, double radius, double *dtab)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x*blockDim.x + threadIdx.x;
    const int q = blockIdx.y;                                 // uniform
    if (t >= n_list) return;
    const int k = swe_ldi(swe_rsrc(cells), (unsigned)t*4u, 0u);
    double px[NPC], py[NPC];
#pragma unroll
    for (int i = 0; i < NPC; i++) {
        const int vid = swe_ldi(swe_rsrc(cv), (unsigned)k*4u, i*stride*4u);
        px[i] = swe_ld(swe_rsrc(vx), (unsigned)vid*8u, 0u);
        py[i] = swe_ld(swe_rsrc(vy), (unsigned)vid*8u, 0u);
    }
    const double x = swe_dfarm_point<NPC>(R.phi + q*NPC, px), y = swe_dfarm_point<NPC>(R.phi + q*NPC, py);
    const double norm = radius*radius*SWE_DFARM_NORM;
    const int j0 = swe_ldi(swe_rsrc(c_off), (unsigned)t*4u, 0u), j1 = swe_ldi(swe_rsrc(c_off), (unsigned)t*4u, 4u);
    double d = 0.0;
    for (int j = j0; j < j1; j++) {
        const int tb = swe_ldi(swe_rsrc(c_idx), (unsigned)j*4u, 0u);
        const double tx = swe_ld(swe_rsrc(txy), (unsigned)tb*16u, 0u), ty = swe_ld(swe_rsrc(txy), (unsigned)tb*16u, 8u);
        d = d + swe_dfarm_psi((x - tx)/radius)*swe_dfarm_psi((y - ty)/radius)/norm;
    }
    swe_st(swe_rsrc(dtab), ((unsigned)q*(unsigned)n_list + (unsigned)t)*8u, 0u, d);
}

// what the drag and the power pass load of a listed cell
template <int NPC>
struct SweDfarmCell {
    double u[NPC], v[NPC], H[NPC], h[NPC], px[NPC], py[NPC];
};
template <int NPC>
__device__ __forceinline__ void swe_dfarm_load(const SweDfarmArgs &a, int k, SweDfarmCell<NPC> &c)
{
#pragma clang fp contract(off)
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = a.stride*8u, S4 = a.stride*4u;
#pragma unroll
    for (int i = 0; i < NPC; i++) {
        c.u[i] = swe_ld(swe_rsrc(a.in), k8, i*S8);
        c.v[i] = swe_ld(swe_rsrc(a.in + (size_t)NPC*a.stride), k8, i*S8);
        const double e = swe_ld(swe_rsrc(a.in + (size_t)2*NPC*a.stride), k8, i*S8);
        const int vid = swe_ldi(swe_rsrc(a.cv), k4, i*S4);
        c.px[i] = swe_ld(swe_rsrc(a.vx), (unsigned)vid*8u, 0u);
        c.py[i] = swe_ld(swe_rsrc(a.vy), (unsigned)vid*8u, 0u);
        c.h[i] = swe_ld(swe_rsrc(a.vh), (unsigned)vid*8u, 0u);
        c.H[i] = a.nonlin ? c.h[i] + e : c.h[i];
    }
}
// det J = d0 + d1 xi + d2 zeta of a quadrilateral (swe_quad_stage_cell); a triangle: d0 = the cell's area (the weights sum to 1)
template <int NPC, bool AFFINE>
__device__ __forceinline__ void swe_dfarm_jacobian(const double px[NPC], const double py[NPC], double &d0, double &d1, double &d2)
{
#pragma clang fp contract(off)
    d1 = d2 = 0.0;
    if constexpr (NPC == 3) {
        d0 = 0.5*((px[1] - px[0])*(py[2] - py[0]) - (px[2] - px[0])*(py[1] - py[0]));
    } else {
        const double ax = px[1] - px[0], ay = py[1] - py[0], bx = px[3] - px[0], by = py[3] - py[0];
        d0 = ax*by - ay*bx;
        if constexpr (!AFFINE) {
            const double cx = (px[0] - px[1]) + (px[2] - px[3]), cy = (py[0] - py[1]) + (py[2] - py[3]);
            d1 = ax*cy - ay*cx;
            d2 = cx*by - cy*bx;
        }
    }
}

template <int NPC, bool AFFINE>
__global__ void __launch_bounds__(SWE_BLOCK) swe_dfarm_drag_kernel(const SweDfarmRule R, const SweDfarmArgs a)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x*SWE_BLOCK + (int)threadIdx.x;
    if (t >= a.n_list) return;
    const int k = swe_ldi(swe_rsrc(a.cells), (unsigned)t*4u, 0u);
    if (k < a.cell_begin || k >= a.cell_end) return;
    const SweFarm &F = *a.F;
    SweDfarmCell<NPC> c;
    swe_dfarm_load<NPC>(a, k, c);
    double d0, d1, d2;
    swe_dfarm_jacobian<NPC, AFFINE>(c.px, c.py, d0, d1, d2);
    double bu[NPC], bv[NPC];
#pragma unroll
    for (int i = 0; i < NPC; i++) bu[i] = bv[i] = 0.0;
    const swe_rsrc_t rd = swe_rsrc(a.dtab);
    const unsigned t8 = (unsigned)t*8u, L8 = (unsigned)a.n_list*8u;
#pragma unroll 1
    for (int q = 0; q < R.n_q; q++) {                         // uniform trip count
        const double *phi = R.phi + q*NPC;
        const double dq = swe_ld(rd, t8, (unsigned)q*L8);
        double uq = 0.0, vq = 0.0, Hq = 0.0;
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            uq = fma(phi[i], c.u[i], uq);
            vq = fma(phi[i], c.v[i], vq);
            Hq = fma(phi[i], c.H[i], Hq);
        }
        double J = d0;
        if constexpr (NPC == 4 && !AFFINE) J = d0 + d1*(phi[1] + phi[2]) + d2*(phi[2] + phi[3]);
        const double s = dq != 0.0 ? R.w[q]*J*swe_farm_drag_pt(F, uq, vq, Hq, dq) : 0.0;     // (outside every bump: no NaN of alpha times 0)
        const double su = s*uq, sv = s*vq;
#pragma unroll
        for (int i = 0; i < NPC; i++) {
            bu[i] -= phi[i]*su;
            bv[i] -= phi[i]*sv;
        }
    }
    // the cell's mass inverse, as the SIPG kernels apply it (swe2d_sipg.h)
    const unsigned k8 = (unsigned)k*8u, S8 = a.stride*8u;
    const swe_rsrc_t rou = swe_rsrc(a.out), rov = swe_rsrc(a.out + (size_t)NPC*a.stride);
    if constexpr (NPC == 3) {
        const double s = 6.0*a.sdt*swe_rcp(2.0*d0);
        const double sbu = bu[0] + bu[1] + bu[2], sbv = bv[0] + bv[1] + bv[2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            swe_st(rou, k8, i*S8, swe_ld(rou, k8, i*S8) + s*(4.0*bu[i] - sbu));
            swe_st(rov, k8, i*S8, swe_ld(rov, k8, i*S8) + s*(4.0*bv[i] - sbv));
        }
    } else if constexpr (AFFINE) {
        const double sc = a.sdt*swe_rcp(d0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            swe_st(rou, k8, i*S8, swe_ld(rou, k8, i*S8) + sc*(16.0*bu[i] - 8.0*bu[(i + 1) & 3] - 8.0*bu[(i + 3) & 3] + 4.0*bu[(i + 2) & 3]));
            swe_st(rov, k8, i*S8, swe_ld(rov, k8, i*S8) + sc*(16.0*bv[i] - 8.0*bv[(i + 1) & 3] - 8.0*bv[(i + 3) & 3] + 4.0*bv[(i + 2) & 3]));
        }
    } else {
        SweQuadMass M;
        SweQuadLDL L;
        swe_quad_mass(d0, d1, d2, M);
        swe_quad_mass_factor(M, L);
        swe_quad_mass_solve(L, bu);
        swe_quad_mass_solve(L, bv);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            swe_st(rou, k8, i*S8, swe_ld(rou, k8, i*S8) + a.sdt*bu[i]);
            swe_st(rov, k8, i*S8, swe_ld(rov, k8, i*S8) + a.sdt*bv[i]);
        }
    }
}

// the power integrand at a point (swe2d_turbine.hip: swe_farm_power_pt, stated here because that unit is not a header)
__device__ __forceinline__ double swe_dfarm_power_pt(const SweFarm &F, double uq, double vq, double hq, double dq)
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

// A lane's running limb sums: every term (one point of one cell) is split exactly and added as integers, the wave's total goes to
// the accumulators once (swe_sum_accumulate does both per term).  The sum of a lane's terms is then exact too: the farm's power
// and the sum of its turbines' powers differ by the rounding of their terms only.
struct SweDfarmLimbs {
    long long q[SWE_SUM_LIMBS] = {0, 0, 0, 0, 0, 0};
    unsigned bad = 0u;
};
__device__ __forceinline__ void swe_dfarm_limbs_add(SweDfarmLimbs &A, double x)
{
    long long q[SWE_SUM_LIMBS];
    swe_sum_split(x, q, A.bad);
#pragma unroll
    for (int j = 0; j < SWE_SUM_LIMBS; j++) A.q[j] += q[j];
}
__device__ __forceinline__ void swe_dfarm_limbs_flush(const SweDfarmLimbs &A, unsigned long long *acc, unsigned long long *bad_counter)
{
#pragma unroll
    for (int j = 0; j < SWE_SUM_LIMBS; j++) {
        long long v = A.q[j];
        for (int off = SWE_BLOCK/2; off > 0; off >>= 1) v += __shfl_down(v, off, SWE_BLOCK);
        if (threadIdx.x == 0 && v != 0) atomicAdd(acc + j, (unsigned long long)v);
    }
    if (A.bad) atomicAdd(bad_counter, 1ull);
}

template <int NPC, bool AFFINE>
__global__ void __launch_bounds__(SWE_BLOCK) swe_dfarm_power_kernel(const SweDfarmRule R, const SweDfarmArgs a)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x*SWE_BLOCK + (int)threadIdx.x;
    const SweFarm &F = *a.F;
    SweDfarmLimbs P;
    if (t < a.n_list) {
        const int k = swe_ldi(swe_rsrc(a.cells), (unsigned)t*4u, 0u);
        SweDfarmCell<NPC> c;
        swe_dfarm_load<NPC>(a, k, c);
        double d0, d1, d2;
        swe_dfarm_jacobian<NPC, AFFINE>(c.px, c.py, d0, d1, d2);
        const swe_rsrc_t rd = swe_rsrc(a.dtab);
        const unsigned t8 = (unsigned)t*8u, L8 = (unsigned)a.n_list*8u;
#pragma unroll 1
        for (int q = 0; q < R.n_q; q++) {
            const double *phi = R.phi + q*NPC;
            const double dq = swe_ld(rd, t8, (unsigned)q*L8);
            double uq = 0.0, vq = 0.0, hq = 0.0;
#pragma unroll
            for (int i = 0; i < NPC; i++) {
                uq = fma(phi[i], c.u[i], uq);
                vq = fma(phi[i], c.v[i], vq);
                hq = fma(phi[i], c.h[i], hq);
            }
            double J = d0;
            if constexpr (NPC == 4 && !AFFINE) J = d0 + d1*(phi[1] + phi[2]) + d2*(phi[2] + phi[3]);
            if (dq != 0.0) swe_dfarm_limbs_add(P, (R.w[q]*J)*swe_dfarm_power_pt(F, uq, vq, hq, dq));
        }
    }
    swe_dfarm_limbs_flush(P, a.row, a.bad);
}

// per-turbine power: block b = turbine b, its lanes stride over the turbine's list positions; the turbine's own bump at the points
template <int NPC, bool AFFINE>
__global__ void __launch_bounds__(SWE_BLOCK) swe_dfarm_turbine_kernel(const SweDfarmRule R, const SweDfarmArgs a, const int *t_off,
                                                                      const int *t_pos, const double *txy, double radius,
                                                                      unsigned long long *tpow)
{
#pragma clang fp contract(off)
    const int tb = blockIdx.x;
    const SweFarm &F = *a.F;
    const int j0 = swe_ldi(swe_rsrc(t_off), (unsigned)tb*4u, 0u), j1 = swe_ldi(swe_rsrc(t_off), (unsigned)tb*4u, 4u);
    const double tx = swe_ld(swe_rsrc(txy), (unsigned)tb*16u, 0u), ty = swe_ld(swe_rsrc(txy), (unsigned)tb*16u, 8u);
    const double norm = radius*radius*SWE_DFARM_NORM;
    SweDfarmLimbs P;
    for (int j = j0 + (int)threadIdx.x; j < j1; j += SWE_BLOCK) {
        const int t = swe_ldi(swe_rsrc(t_pos), (unsigned)j*4u, 0u);
        const int k = swe_ldi(swe_rsrc(a.cells), (unsigned)t*4u, 0u);
        SweDfarmCell<NPC> c;
        swe_dfarm_load<NPC>(a, k, c);
        double d0, d1, d2;
        swe_dfarm_jacobian<NPC, AFFINE>(c.px, c.py, d0, d1, d2);
#pragma unroll 1
        for (int q = 0; q < R.n_q; q++) {
            const double *phi = R.phi + q*NPC;
            const double x = swe_dfarm_point<NPC>(phi, c.px), y = swe_dfarm_point<NPC>(phi, c.py);
            const double dq = swe_dfarm_psi((x - tx)/radius)*swe_dfarm_psi((y - ty)/radius)/norm;
            double uq = 0.0, vq = 0.0, hq = 0.0;
#pragma unroll
            for (int i = 0; i < NPC; i++) {
                uq = fma(phi[i], c.u[i], uq);
                vq = fma(phi[i], c.v[i], vq);
                hq = fma(phi[i], c.h[i], hq);
            }
            double J = d0;
            if constexpr (NPC == 4 && !AFFINE) J = d0 + d1*(phi[1] + phi[2]) + d2*(phi[2] + phi[3]);
            if (dq != 0.0) swe_dfarm_limbs_add(P, (R.w[q]*J)*swe_dfarm_power_pt(F, uq, vq, hq, dq));
        }
    }
    unsigned long long *acc = tpow + (size_t)tb*(SWE_SUM_LIMBS + 1);
    swe_dfarm_limbs_flush(P, acc, acc + SWE_SUM_LIMBS);
}

namespace {

void dfarm_fill(Handle *h, const Handle::Farm &f, int m, SweDfarmRule &R, SweDfarmArgs &a)
{
    std::memcpy(R.phi, f.phi, sizeof(R.phi));
    std::memcpy(R.w, f.w, sizeof(R.w));
    R.n_q = f.n_q;
    a = SweDfarmArgs{};
    a.F = &h->farm_table.get()->f[m];
    a.stride = (unsigned)h->stride;
    a.cells = f.cells; a.dtab = f.dtab; a.n_list = f.n_list;
    a.cv = h->cv; a.vx = h->vx; a.vy = h->vy; a.vh = h->vh;
    a.nonlin = h->par.use_nonlinear_equations ? 1 : 0;
}

// the instance of a kernel template <NPC, AFFINE> for the handle's cells
#define DFARM_PICK(h, kern) ((h)->npc == 3 ? kern<3, true> : ((h)->affine ? kern<4, true> : kern<4, false>))

}  // namespace

int swe2d_impl::dfarm_launch_drag(Handle *h, int in, int out, double beta, int c0, int c1)
{
    for (int m = 0; m < SWE2D_MAX_FARMS; m++) {
        const Handle::Farm &f = h->farms[m];
        if (!f.live || !f.discrete || f.n_list == 0) continue;
        SweDfarmRule R;
        SweDfarmArgs a;
        dfarm_fill(h, f, m, R, a);
        a.in = h->state[in];
        a.out = h->state[out];
        a.cell_begin = c0; a.cell_end = c1;
        a.sdt = beta*h->par.dt;
        SWE_CHK_SYNC(h->stream);
        hipLaunchKernelGGL(DFARM_PICK(h, swe_dfarm_drag_kernel), dim3((f.n_list + SWE_BLOCK - 1)/SWE_BLOCK), dim3(SWE_BLOCK), 0, h->stream, R, a);
        HIP_TRY(h, hipGetLastError());
    }
    return SWE2D_OK;
}

int swe2d_impl::dfarm_launch_power(Handle *h, unsigned long long *row)
{
    for (int m = 0; m < SWE2D_MAX_FARMS; m++) {
        const Handle::Farm &f = h->farms[m];
        if (!f.live || !f.discrete || f.n_list == 0) continue;
        SweDfarmRule R;
        SweDfarmArgs a;
        dfarm_fill(h, f, m, R, a);
        a.in = h->state[0];
        a.row = row + (size_t)m*SWE_SUM_LIMBS;
        a.bad = row + SWE_MAX_FARMS*SWE_SUM_LIMBS;
        SWE_CHK_SYNC(h->stream);
        hipLaunchKernelGGL(DFARM_PICK(h, swe_dfarm_power_kernel), dim3((f.n_list + SWE_BLOCK - 1)/SWE_BLOCK), dim3(SWE_BLOCK), 0, h->stream, R, a);
        HIP_TRY(h, hipGetLastError());
    }
    return SWE2D_OK;
}

extern "C" {

int swe2d_dfarm_set(swe2d_handle *hh, int32_t farm, const swe2d_turbine_params *p, int32_t n_turbines, const double *xy,
                    const uint8_t *cell_mask, int32_t n_q, const double *phi, const double *w)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_dfarm_set: discrete turbine farms are not available with wetting-drying");
    if (farm < 0 || farm >= SWE2D_MAX_FARMS) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: farm must be in 0 .. SWE2D_MAX_FARMS-1");
    if (!p || !cell_mask || !phi || !w || (n_turbines > 0 && !xy)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: null argument");
    if (n_turbines < 0 || n_turbines > (1 << 20)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: bad number of turbines");
    if (n_q < 1 || n_q > SWE2D_MAX_FARM_QUAD) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: n_q must be in 1 .. SWE2D_MAX_FARM_QUAD");
    if (p->n_table < 0 || p->n_table == 1 || p->n_table > SWE2D_MAX_THRUST_TABLE)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: n_table must be 0 or 2 .. SWE2D_MAX_THRUST_TABLE");
    for (int j = 0; j + 1 < p->n_table; j++)
        if (!(p->speeds[j + 1] > p->speeds[j])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: thrust speeds must increase strictly");
    if (!(p->projected_diameter > 0.0) || !(p->rotor_area > 0.0) || !std::isfinite(p->projected_diameter))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: diameters must be positive");
    for (int i = 0; i < n_q*h->npc; i++)
        if (!std::isfinite(phi[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: the rule must be finite");
    for (int i = 0; i < n_q; i++)
        if (!(w[i] > 0.0) || !std::isfinite(w[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: the weights must be positive");
    for (int i = 0; i < 2*n_turbines; i++)
        if (!std::isfinite(xy[i])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_set: turbine coordinates must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                          // launches that read the slot's tables are done
    // ---- the lists, on the host, from the mesh as the device holds it
    const int npc = h->npc, nc = h->n_cells;
    const size_t S = h->stride;
    std::vector<int> cv((size_t)npc*S);
    std::vector<double> vx(h->n_vertices), vy(h->n_vertices);
    HIP_TRY(h, hipMemcpy(cv.data(), h->cv, cv.size()*sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(vx.data(), h->vx, vx.size()*sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(vy.data(), h->vy, vy.size()*sizeof(double), hipMemcpyDeviceToHost));
    const double r = 0.5*p->projected_diameter;
    std::vector<int> list, c_off(1, 0), c_idx;
    if (n_turbines > 0) {
        for (int k = 0; k < h->n_owned && k < nc; k++) {
            if (!cell_mask[k]) continue;
            double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
            for (int i = 0; i < npc; i++) {
                const int vid = cv[(size_t)i*S + k];
                const double x = vx[vid], y = vy[vid];
                if (i == 0) { x0 = x1 = x; y0 = y1 = y; }
                x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            }
            const size_t before = c_idx.size();
            for (int t = 0; t < n_turbines; t++)
                if (x0 < xy[2*t] + r && x1 > xy[2*t] - r && y0 < xy[2*t + 1] + r && y1 > xy[2*t + 1] - r) c_idx.push_back(t);
            if (c_idx.size() > before) { list.push_back(k); c_off.push_back((int)c_idx.size()); }
        }
    }
    const int n_list = (int)list.size(), nnz = (int)c_idx.size();
    if ((size_t)n_list*(size_t)n_q >= ((size_t)1 << 28))
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_dfarm_set: the density table would not fit 32-bit byte offsets");
    std::vector<int> t_off((size_t)n_turbines + 1, 0), t_pos(nnz);
    for (int j = 0; j < nnz; j++) t_off[c_idx[j] + 1]++;
    for (int t = 0; t < n_turbines; t++) t_off[t + 1] += t_off[t];
    {
        std::vector<int> fill(t_off.begin(), t_off.end() - 1);
        for (int c = 0; c < n_list; c++)
            for (int j = c_off[c]; j < c_off[c + 1]; j++) t_pos[fill[c_idx[j]]++] = c;
    }
    // ---- the new slot, built aside: a failure leaves the handle as it was
    Handle::Farm f;
    f.discrete = true;
    f.par = *p;
    f.n_q = n_q; f.n_turbines = n_turbines; f.radius = r; f.n_list = n_list; f.nnz = nnz;
    std::memcpy(f.phi, phi, (size_t)n_q*npc*sizeof(double));
    std::memcpy(f.w, w, (size_t)n_q*sizeof(double));
    if (n_turbines > 0) {
        HIP_TRY(h, f.txy.alloc((size_t)2*n_turbines));
        HIP_TRY(h, hipMemcpy(f.txy, xy, (size_t)2*n_turbines*sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, f.tpow.alloc((size_t)n_turbines*(SWE_SUM_LIMBS + 1)));
    }
    if (n_list > 0) {
        HIP_TRY(h, f.cells.alloc(n_list));
        HIP_TRY(h, hipMemcpy(f.cells, list.data(), (size_t)n_list*sizeof(int), hipMemcpyHostToDevice));
        const size_t n_int = (size_t)n_list + 1 + nnz + n_turbines + 1 + nnz;
        HIP_TRY(h, f.csr.alloc(n_int));
        int *d = f.csr;
        HIP_TRY(h, hipMemcpy(d, c_off.data(), ((size_t)n_list + 1)*sizeof(int), hipMemcpyHostToDevice)); d += n_list + 1;
        HIP_TRY(h, hipMemcpy(d, c_idx.data(), (size_t)nnz*sizeof(int), hipMemcpyHostToDevice)); d += nnz;
        HIP_TRY(h, hipMemcpy(d, t_off.data(), ((size_t)n_turbines + 1)*sizeof(int), hipMemcpyHostToDevice)); d += n_turbines + 1;
        HIP_TRY(h, hipMemcpy(d, t_pos.data(), (size_t)nnz*sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(h, f.dtab.alloc((size_t)n_q*n_list));
        SweDfarmRule R;
        std::memcpy(R.phi, f.phi, sizeof(R.phi));
        std::memcpy(R.w, f.w, sizeof(R.w));
        R.n_q = n_q;
        const dim3 grid(grid_for(n_list), n_q);
        SWE_CHK_SYNC(h->stream);
        if (npc == 4)
            hipLaunchKernelGGL(swe_dfarm_density_kernel<4>, grid, dim3(256), 0, h->stream, R, f.cells, n_list, (unsigned)S, h->cv, h->vx, h->vy,
                               f.csr, f.csr + n_list + 1, f.txy, r, f.dtab);
        else
            hipLaunchKernelGGL(swe_dfarm_density_kernel<3>, grid, dim3(256), 0, h->stream, R, f.cells, n_list, (unsigned)S, h->cv, h->vx, h->vy,
                               f.csr, f.csr + n_list + 1, f.txy, r, f.dtab);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (!h->farm_rows) { if (int rc = farm_rows_alloc(h, 0)) return rc; }
    f.live = true;
    std::swap(h->farms[farm], f);                                         // `f` takes what the slot held with it
    return farm_upload_table(h);
}

int swe2d_dfarm_density_read(swe2d_handle *hh, int32_t farm, int32_t *n_list, int32_t *n_q, int32_t *cells_out, double *density_out)
{
    Handle *h = H(hh);
    if (!h || !n_list || !n_q) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (farm < 0 || farm >= SWE2D_MAX_FARMS || !h->farms[farm].live || !h->farms[farm].discrete)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_density_read: not a discrete farm");
    const Handle::Farm &f = h->farms[farm];
    *n_list = f.n_list; *n_q = f.n_q;
    if (f.n_list == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (cells_out) HIP_TRY(h, hipMemcpy(cells_out, f.cells, (size_t)f.n_list*sizeof(int), hipMemcpyDeviceToHost));
    if (density_out) HIP_TRY(h, hipMemcpy(density_out, f.dtab, (size_t)f.n_q*f.n_list*sizeof(double), hipMemcpyDeviceToHost));
    return SWE2D_OK;
}

int swe2d_dfarm_turbine_power(swe2d_handle *hh, int32_t farm, double *out)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (farm_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "turbine farm calls are not allowed inside a stream capture");
    if (farm < 0 || farm >= SWE2D_MAX_FARMS || !h->farms[farm].live || !h->farms[farm].discrete)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_dfarm_turbine_power: not a discrete farm");
    const Handle::Farm &f = h->farms[farm];
    if (f.n_turbines == 0) return SWE2D_OK;
    if (!out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    if (int rc = capture_parity_check(h)) return rc;
    for (int t = 0; t < f.n_turbines; t++) out[t] = 0.0;
    if (f.n_list == 0) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n_acc = (size_t)f.n_turbines*(SWE_SUM_LIMBS + 1);
    HIP_TRY(h, hipMemsetAsync(f.tpow, 0, n_acc*sizeof(unsigned long long), h->stream));
    SweDfarmRule R;
    SweDfarmArgs a;
    dfarm_fill(h, f, farm, R, a);
    a.in = h->state[0];
    const int *t_off = f.csr + f.n_list + 1 + f.nnz;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(DFARM_PICK(h, swe_dfarm_turbine_kernel), dim3(f.n_turbines), dim3(SWE_BLOCK), 0, h->stream, R, a, t_off,
                       t_off + f.n_turbines + 1, f.txy, f.radius, f.tpow);
    HIP_TRY(h, hipGetLastError());
    std::vector<unsigned long long> host(n_acc);
    HIP_TRY(h, hipMemcpyAsync(host.data(), f.tpow, n_acc*sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = flow_check(h)) return rc;
    for (int t = 0; t < f.n_turbines; t++) {
        const unsigned long long *acc = host.data() + (size_t)t*(SWE_SUM_LIMBS + 1);
        if (acc[SWE_SUM_LIMBS] != 0) return fail(h, SWE2D_ERR_NOT_FINITE, "turbine power is not finite");
        int64_t limbs[SWE_SUM_LIMBS];
        for (int j = 0; j < SWE_SUM_LIMBS; j++) limbs[j] = (int64_t)acc[j];
        out[t] = swe2d_sum_limbs_to_double(limbs);
    }
    return SWE2D_OK;
}

}  // extern "C"
