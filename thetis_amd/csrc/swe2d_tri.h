// swe2d_tri.h - the arithmetic of ONE triangle cell in one SSPRK33 stage, written once (included by swe2d_kernels.h).
//
// Every way of launching a step - three stage launches (swe_stage_kernel, all its variants), the dataflow kernel (swe2d_flow.h),
// the fused stage pair and the three-stage kernel (swe2d_fuse.h) - must give the same bits.  They do because they call the same
// functions: cell integrals (swe_tri_cell), one interior facet (swe_tri_facet), mass inverse + Shu-Osher combine + boundary pass +
// wetting-drying finish (swe_tri_finish), and the correction a boundary facet adds to finished outputs (swe_tri_boundary_correct,
// shared with swe_boundary_epilogue).  What differs between the kernels stays with them: where the values come from (registers,
// LDS, granules), what is kept between stages, and when the loads are issued.
// No implicit contraction anywhere in this file: which of two products the compiler fuses depends on the code around it, so every
// fused multiply-add is written out and EVERY function here, however small, carries `fp contract(off)` - the pragma is lexical, it
// does not follow a call, and an operation that may be contracted stays so where the optimiser merges it with a caller's copy.
// (The one copy of these formulas outside this file, the VISC branch of swe_stage_kernel, stands under that kernel's own pragma.)
#pragma once

// nodal total depth: the displaced depth D the planes hold with wetting-drying, else h + eta or, for the linear equations, h
template <bool NONLIN, bool WD>
__device__ __forceinline__ double swe_tri_depth(double h, double e, double D)
{
#pragma clang fp contract(off)
    return WD ? D : (NONLIN ? h + e : h);
}
template <bool NONLIN, bool WD>
__device__ __forceinline__ void swe_tri_depths(const double h[3], const double e[3], const double *D, double H[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; i++) H[i] = swe_tri_depth<NONLIN, WD>(h[i], e[i], WD ? D[i] : 0.0);
}

// A*grad(phi_i) = -nF_{i+1}/2, from the scaled outward normals nF_f = |F| n of facet f (vertex f -> f+1; counter-clockwise cell)
__device__ __forceinline__ void swe_tri_grad(const double nx[3], const double ny[3], double gxs[3], double gys[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; i++) {
        gxs[i] = -0.5*nx[(i + 1) % 3];
        gys[i] = -0.5*ny[(i + 1) % 3];
    }
}

__device__ __forceinline__ void swe_tri_facet_len(double nxs, double nys, double &L, double &rL)
{
#pragma clang fp contract(off)
    swe_sqrt_rsqrt(swe_dot2(nxs, nxs, nys, nys), L, rL);
}

// ---- cell integrals (closed form).  e: elevation, H: nodal total depth (swe_tri_depth)
template <bool NONLIN>
__device__ __forceinline__ void swe_tri_cell(double g, const double u[3], const double v[3], const double e[3], const double H[3],
                                             const double nx[3], const double ny[3], double bu[3], double bv[3], double be[3])
{
#pragma clang fp contract(off)
    double gxs[3], gys[3];
    swe_tri_grad(nx, ny, gxs, gys);
    const double ge3 = g*(e[0] + e[1] + e[2])*(1.0/3.0);
    const double SHu = swe_int2(H, u)*(1.0/12.0), SHv = swe_int2(H, v)*(1.0/12.0);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        bu[i] = gxs[i]*ge3;                              // +g eta div(psi)       shallowwater_eq.py:361
        bv[i] = gys[i]*ge3;
        be[i] = swe_dot2(gxs[i], SHu, gys[i], SHv);      // +grad(phi).(H u)      shallowwater_eq.py:422
    }
    if (NONLIN) {                                        // +(psi div u + u.grad psi).u  shallowwater_eq.py:478
        const double Suu = swe_int2(u, u)*(1.0/12.0), Suv = swe_int2(u, v)*(1.0/12.0), Svv = swe_int2(v, v)*(1.0/12.0);
        const double D12 = fma(gys[2], v[2], fma(gys[1], v[1], fma(gys[0], v[0],
                           fma(gxs[2], u[2], fma(gxs[1], u[1], gxs[0]*u[0])))))*(1.0/12.0);
        const double us = u[0] + u[1] + u[2], vs = v[0] + v[1] + v[2];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            bu[i] = fma(gys[i], Suv, fma(gxs[i], Suu, fma(D12, us + u[i], bu[i])));
            bv[i] = fma(gys[i], Svv, fma(gxs[i], Suv, fma(D12, vs + v[i], bv[i])));
        }
    }
}

// ---- one facet (nodes a -> b of this cell): 2-point Gauss-Legendre, numerical fluxes seen from this cell, accumulated into the
// residuals of its two nodes.  (.)na / (.)nb: the neighbour's values on my nodes a / b; dna, dnb: what its elevation planes hold
// there - eta, or with wetting-drying its nodal depth D, from which its elevation follows by the closed form (bathymetry and alpha
// are continuous: same vertices).  Ha, Hb, ala, alb: wetting-drying only.
// bnd: a boundary facet.  It carries finite "neighbour" traces (the callers point it at the cell itself), its flux is evaluated like
// any other and discarded: the boundary pass of swe_tri_finish / swe_boundary_epilogue adds the facet's true flux to the finished
// outputs.  (Branch-free on purpose, see swe_stage_kernel; SKIPB: the variants that branch round the evaluation all the same.)
// WAVEB: the six zero assignments sit behind a wave-uniform test, wave_bnd = __any(a lane of the wave has a boundary facet), which the
// caller forms once per cell body - a wave without one branches round them on the scalar unit instead of issuing six moves with an
// empty mask and the test of bnd per facet (the three-stage kernel of swe2d_fuse.h: 5425 of the bench mesh's 5733 tiles have no wall
// cell).  Every lane's fluxes are what they were: zeros with bnd, untouched without.
template <bool NONLIN, bool LF, bool WD, bool SKIPB = false, bool WAVEB = false>
__device__ __forceinline__ void swe_tri_facet(double g, double sigma_lf, bool bnd, double ua, double ub, double va, double vb, double ea,
                                              double eb, double ha, double hb, double Ha, double Hb, double ala, double alb, double una,
                                              double unb, double vna, double vnb, double dna, double dnb, double nxs, double nys, double L,
                                              double rL, double &bua, double &bub, double &bva, double &bvb, double &bea, double &beb,
                                              bool wave_bnd = true)
{
#pragma clang fp contract(off)
    double Fau = 0.0, Fbu = 0.0, Fav = 0.0, Fbv = 0.0, Fae = 0.0, Fbe = 0.0;
    if (!SKIPB || !bnd) {
        const double ena = WD ? swe_wd_eta(dna, ha, ala) : dna, enb = WD ? swe_wd_eta(dnb, hb, alb) : dnb;
        swe_facet_flux<NONLIN, LF, WD>(g, sigma_lf, ua, ub, va, vb, ea, eb, ha, hb, Ha, Hb, una, unb, vna, vnb, ena, enb, dna, dnb, nxs, nys,
                                       L, rL, Fau, Fbu, Fav, Fbv, Fae, Fbe);
    }
    if constexpr (WAVEB) {
        if (wave_bnd) {
            asm volatile("");                                  // keeps the block a block: without it the moves are hoisted and the branch goes
            if (bnd) { Fau = 0.0; Fbu = 0.0; Fav = 0.0; Fbv = 0.0; Fae = 0.0; Fbe = 0.0; }
        }
    } else if (bnd) { Fau = 0.0; Fbu = 0.0; Fav = 0.0; Fbv = 0.0; Fae = 0.0; Fbe = 0.0; }
    bua = fma(-0.5, Fau, bua); bub = fma(-0.5, Fbu, bub);
    bva = fma(-0.5, Fav, bva); bvb = fma(-0.5, Fbv, bvb);
    bea = fma(-0.5, Fae, bea); beb = fma(-0.5, Fbe, beb);
}

// ---- what the flux F of a boundary facet (nodes a -> b) adds to the finished outputs: sfac * M^-1 of a vector that is non-zero at
// nodes a and b only (4 d_i - (d_a + d_b)), d = -F/2, sfac = 6 dt beta / (2A); static output indices
__device__ __forceinline__ void swe_tri_boundary_correct(double sfac, int a, int b, double Fau, double Fbu, double Fav, double Fbv,
                                                         double Fae, double Fbe, double ou[3], double ov[3], double oe[3])
{
#pragma clang fp contract(off)
    const double dau = -0.5*Fau, dbu = -0.5*Fbu, dav = -0.5*Fav, dbv = -0.5*Fbv, dae = -0.5*Fae, dbe = -0.5*Fbe;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double wa = (i == a) ? 3.0 : -1.0, wb = (i == b) ? 3.0 : -1.0;
        ou[i] = fma(sfac, fma(wa, dau, wb*dbu), ou[i]);
        ov[i] = fma(sfac, fma(wa, dav, wb*dbv), ov[i]);
        oe[i] = fma(sfac, fma(wa, dae, wb*dbe), oe[i]);
    }
}

// ---- mass inverse (M^-1 b)_i = 3/A (4 b_i - sum b), times dt beta, and the Shu-Osher combine with w = a0*U0 + a1*U_in; then the
// boundary facets named in bmarkers (8 bits of marker per facet, 0: none; bkind1: the table entry of the first one, fetched by the
// caller with its other loads); then, with wd_fin, zeta = D - h -> the limited depth D the planes hold and the dry-ground relaxation.
// e: elevation; Dn, al: wetting-drying only (nodal depth, alpha).
// GEOM: what becomes of 1/twoA, a pure function of the mesh - SWE_GEOM_COMPUTE: evaluated here; SWE_GEOM_KEEP: evaluated here and left
// in the lane's LDS record, geo[6*PLANE]; SWE_GEOM_STORED: taken from the record a SWE_GEOM_KEEP call filled - the value that
// instruction sequence gave, so the same bits (the three-stage kernel of swe2d_fuse.h; swe_flow_rhs_facets does the same for the
// facet lengths).
// Boundary facets are < 0.3 % of the work but their code needs ~60 registers of temporaries, so they are evaluated here, after the
// outputs are finished and the working set of the facet loop is dead, from the values the lane still holds: every lane works on
// ITS boundary facet, in ascending facet order - a wave runs the boundary code once (twice where a corner cell is among its lanes),
// not once per facet slot.
// (WALLFAST: the closed-wall path of swe_boundary_facet)
#define SWE_GEOM_COMPUTE 0
#define SWE_GEOM_KEEP 1
#define SWE_GEOM_STORED 2
template <bool NONLIN, bool LF, bool WD, bool WALLFAST, int GEOM = SWE_GEOM_COMPUTE, int PLANE = SWE_BLOCK>
__device__ __forceinline__ void swe_tri_finish(const SweStageArgs &p, int k, double beta, double twoA, const double u[3], const double v[3],
                                               const double e[3], const double h[3], const double *Dn, const double *al,
                                               const double nx[3], const double ny[3], int bmarkers, int bkind1, const double bu[3],
                                               const double bv[3], const double be[3], const double wu[3], const double wv[3],
                                               const double we[3], bool wd_fin, double ou[3], double ov[3], double oe[3],
                                               double *geo = nullptr)
{
#pragma clang fp contract(off)
    const double dtb6 = 6.0*p.dt*beta;
    double rA;
    if constexpr (GEOM == SWE_GEOM_STORED) rA = geo[6*PLANE];
    else rA = swe_rcp(twoA);
    if constexpr (GEOM == SWE_GEOM_KEEP) geo[6*PLANE] = rA;
    const double s = dtb6*rA;
    const double su = bu[0] + bu[1] + bu[2], sv = bv[0] + bv[1] + bv[2], se = be[0] + be[1] + be[2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ou[i] = fma(s, fma(4.0, bu[i], -su), wu[i]);
        ov[i] = fma(s, fma(4.0, bv[i], -sv), wv[i]);
        oe[i] = fma(s, fma(4.0, be[i], -se), we[i]);          // eta, or zeta = D - h with wetting-drying
    }
    if (bmarkers != 0) {
        // 2A as swe_boundary_epilogue forms it (swe_cross2a), from the facet normals: x1 - x0 = -ny[0], y2 - y0 = -nx[2],
        // y1 - y0 = nx[0], x2 - x0 = ny[2] (negation is exact)
        const double sfac = 6.0*p.dt*beta*swe_rcp(fma(-ny[0], -nx[2], -(nx[0]*ny[2])));
        int rem = ((bmarkers & 0xff) ? 1 : 0) | ((bmarkers & 0xff00) ? 2 : 0) | ((bmarkers & 0xff0000) ? 4 : 0);
        int kind_next = bkind1;                     // first pass: prefetched; a second pass (corner cell) reads the table
        // scalars, not the parameter arrays: a select between loads through a pointer parameter becomes a load from a selected
        // address and the arrays end up in scratch
        const double u_0 = u[0], u_1 = u[1], u_2 = u[2], v_0 = v[0], v_1 = v[1], v_2 = v[2], e_0 = e[0], e_1 = e[1], e_2 = e[2];
        const double h_0 = h[0], h_1 = h[1], h_2 = h[2], nx_0 = nx[0], nx_1 = nx[1], nx_2 = nx[2], ny_0 = ny[0], ny_1 = ny[1], ny_2 = ny[2];
        const double D_0 = WD ? Dn[0] : 0.0, D_1 = WD ? Dn[1] : 0.0, D_2 = WD ? Dn[2] : 0.0;
        const double al_0 = WD ? al[0] : 0.0, al_1 = WD ? al[1] : 0.0, al_2 = WD ? al[2] : 0.0;
#define SWE_SEL3(x, i) ((i) == 0 ? x##_0 : ((i) == 1 ? x##_1 : x##_2))
#pragma unroll 1
        while (rem) {
            const int f = (rem & 1) ? 0 : ((rem & 2) ? 1 : 2);
            rem &= rem - 1;
            const int a = f, b = (f == 2) ? 0 : f + 1;
            const double nxs = SWE_SEL3(nx, f), nys = SWE_SEL3(ny, f);
            double L, rL;
            swe_tri_facet_len(nxs, nys, L, rL);
            double Fau = 0.0, Fbu = 0.0, Fav = 0.0, Fbv = 0.0, Fae = 0.0, Fbe = 0.0;
            const double Ha = swe_tri_depth<NONLIN, WD>(SWE_SEL3(h, a), SWE_SEL3(e, a), SWE_SEL3(D, a));
            const double Hb = swe_tri_depth<NONLIN, WD>(SWE_SEL3(h, b), SWE_SEL3(e, b), SWE_SEL3(D, b));
            swe_boundary_facet<NONLIN, LF, WD, WALLFAST>(p, (bmarkers >> (8*f)) & 0xff, k, a, b, SWE_SEL3(u, a), SWE_SEL3(u, b), SWE_SEL3(v, a),
                                                         SWE_SEL3(v, b), SWE_SEL3(e, a), SWE_SEL3(e, b), SWE_SEL3(h, a), SWE_SEL3(h, b), Ha, Hb,
                                                         SWE_SEL3(al, a), SWE_SEL3(al, b), nxs, nys, L, rL, Fau, Fbu, Fav, Fbv, Fae, Fbe, kind_next);
            kind_next = -1;
            swe_tri_boundary_correct(sfac, a, b, Fau, Fbu, Fav, Fbv, Fae, Fbe, ou, ov, oe);
        }
#undef SWE_SEL3
    }
    if (WD && wd_fin) swe_wd_finish<3>(p.g, beta*p.dt, h, al, ou, ov, oe, !p.wd_skip_relax);
}
