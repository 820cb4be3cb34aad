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
// swe_bedload_kernel         - with a bedload model (swe2d_bedload_set), once per time step after the flow, sediment and limiter passes, one
//                               lane per cell: Meyer-Peter-Mueller transport q_b at the cell's three nodes with the slope and secondary
//                               current corrections (include/swe2d.h has the formulas), from the cell's nodal uv and H and the cell-constant
//                               gradients of the bed and of the free surface; then the cell's three contributions to the divergence of q_b
//                               tested with the vertex hat functions, boundary integral of the open facets included.  Written: six q_b
//                               planes and three contribution planes, which the Exner gather adds up per vertex in list order.
// swe_slide_kernel           - with the sediment slide (swe2d_slide_set), once per time step after the bedload pass, one lane per cell:
//                               the slope of the bed from the cell's three vertex beds and the gradient table, the reference's diffusion
//                               coefficient alpha where the slope exceeds the angle of repose (include/swe2d.h has the formulas), and the
//                               cell's three contributions A*alpha*(grad psi_i . grad b).  Written: the alpha and beta planes and three
//                               contribution planes, which the Exner gather adds up per vertex as a sum of its own.  One asin and one cos
//                               from the device's math library; the largest beta of the pass and the count of flagged cells go to two
//                               device words, one atomic each per wave that has something to report.
// The last three and the contribution planes are + - * / in a fixed order without contraction: thetis_amd/sediment_model.py (HostSediment) gives their bits from the
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
    const double *contrib;                      // Exner with bedload: the contribution planes [3][S]
    const double *slide;                        // Exner with slide: its contribution planes [3][S]
    unsigned *count;
    size_t stride;
    int begin, end;                             // cell range / list length / vertices
    int nonlinear, conservative;
    unsigned eq_markers;
    double dtf, min_depth;                      // Exner: dt*fac, the floor of the depth
    double dt;                                  // Exner with slide: the step itself (the slide is not scaled by fac)
    swe2d_sediment_params par;
};

// squared speed, friction coefficient and skin friction ratio at one node: shared by the suspended load and the bedload closures
__device__ __forceinline__ void swe_sediment_friction(double ks, double ksp, double kappa, double u, double v, double H,
                                                      double &unorm, double &qfc, double &mu)
{
#pragma clang fp contract(off)
    unorm = u*u + v*v;
    const double hc = H > 0.001 ? H : 0.001;
    const double ax = 11.036*hc/ks;
    const double aux = ax > 1.001 ? ax : 1.001;
    const double lq = log(aux)/kappa;
    qfc = 2.0/(lq*lq);
    const bool deep = H > ksp;
    const double lc = (1.0/kappa)*log(11.036*(deep ? H : ksp)/ksp);
    const double cfactor = deep ? 2.0/(lc*lc) : 0.0;
    mu = qfc > 0.0 ? cfactor/qfc : 0.0;
}

__device__ __forceinline__ void swe_sediment_erosion(const swe2d_sediment_params &p, double unorm, double qfc, double mu, double H,
                                                     double &E, double &D, double &ceq);

// the closures at one node (include/swe2d.h, swe2d_sediment_params); no argument of log / pow / sqrt leaves its domain on any branch
__device__ __forceinline__ void swe_sediment_closures(const swe2d_sediment_params &p, double u, double v, double H,
                                                      double &E, double &D, double &ceq)
{
#pragma clang fp contract(off)
    double unorm, qfc, mu;
    swe_sediment_friction(p.ks, p.ksp, p.kappa, u, v, H, unorm, qfc, mu);
    swe_sediment_erosion(p, unorm, qfc, mu, H, E, D, ceq);
}

// ... and what follows the friction: Rouse profile, erosion flux, deposition coefficient
__device__ __forceinline__ void swe_sediment_erosion(const swe2d_sediment_params &p, double unorm, double qfc, double mu, double H,
                                                     double &E, double &D, double &ceq)
{
#pragma clang fp contract(off)
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

struct SweBedArgs {
    const double *state;                        // buffer A
    const int *cv, *nbr;
    const double *vh;
    const double *grad;                         // d psi/dx [3][S] | d psi/dy [3][S]
    const double *area;
    double *planes;                             // qbx [3][S] | qby [3][S] | contribution [3][S]
    double *sed_planes;                         // COEF: E [3][S] | D [3][S] | equilibrium [3][S] of the sediment field
    size_t stride;
    int n_cells, nonlinear;
    double g;
    swe2d_bedload_params par;
    swe2d_sediment_params sed;                  // COEF
};

// q_b at one node (include/swe2d.h, swe2d_bedload_params).  `moves` implies U2 > 0, stress > 0 and mu > 0, and every divisor that can
// vanish elsewhere is replaced by 1 there: no division, root or logarithm sees an argument outside its domain on any branch.
template <bool MAG, bool ANG, bool SEC>
__device__ __forceinline__ void swe_bedload_transport(const swe2d_bedload_params &p, double g, double u, double v, double H, double unorm,
                                                      double qfc, double mu, double hx, double hy, double ex, double ey, double &qx, double &qy)
{
#pragma clang fp contract(off)
    const double stress = p.rho0*0.5*qfc*unorm;
    const double thetaprime = mu*stress/p.shields_den;
    const bool moves = thetaprime > p.thetacr;
    const double x = moves ? thetaprime - p.thetacr : 0.0;
    const double phi = moves ? 8.0*x*sqrt(x) : 0.0;
    const double sn = moves ? sqrt(unorm) : 1.0;
    const double calfa = u/sn, salfa = v/sn;
    const double slopecoef = MAG ? 1.0 + p.beta*(hx*calfa + hy*salfa) : 1.0;
    double ca = calfa, sa = salfa;
    if (ANG) {
        const double cparam = p.shields_den*(p.surbeta2*p.surbeta2);
        const double tt1 = sqrt(cparam/(stress > 1e-10 ? stress : 1e-10));
        const double aa = salfa + tt1*hy, bb = calfa + tt1*hx;
        const double comb = sqrt(aa*aa + bb*bb);
        const double nrm = comb > 1e-10 ? comb : 1e-10;
        ca = bb/nrm;
        sa = aa/nrm;
    }
    double factor = slopecoef;
    bool live = phi > 0.0;
    if (SEC) {
        const double vs = u*ey - v*ex;
        const double tdf = 7.0*g*p.rho0*H*qfc/(2.0*p.alpha_secc*(moves ? unorm : 1.0));
        const double t1 = stress*slopecoef*ca + v*tdf*vs;
        const double t2 = stress*slopecoef*sa - u*tdf*vs;
        const double t4 = sqrt(t1*t1 + t2*t2);
        const double t4s = t4 > 0.0 ? t4 : 1.0;
        factor = t4/(moves ? stress : 1.0);
        ca = t1/t4s;
        sa = t2/t4s;
        live = live && t4 > 0.0;
    }
    const double qtot = factor*phi*p.qb_scale;
    qx = live ? qtot*ca : 0.0;
    qy = live ? qtot*sa : 0.0;
}

// COEF: the launch is the sediment field's coefficient pass as well (E, D, equilibrium as swe_sediment_coeff_kernel writes them), the
// friction closures evaluated once per node for both; the host takes it only where both models hold the same ks, ksp and kappa
template <bool MAG, bool ANG, bool SEC, bool COEF>
__global__ void __launch_bounds__(256) swe_bedload_kernel(SweBedArgs a)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x*256 + threadIdx.x;
    if (k >= a.n_cells) return;
    const size_t S = a.stride;
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t ru = swe_rsrc(a.state), rv = swe_rsrc(a.state + 3*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv),
                     rh = swe_rsrc(a.vh), rn = swe_rsrc(a.nbr), rgx = swe_rsrc(a.grad), rgy = swe_rsrc(a.grad + 3*S), ra = swe_rsrc(a.area);
    const swe_rsrc_t ox = swe_rsrc(a.planes), oy = swe_rsrc(a.planes + 3*S), oc = swe_rsrc(a.planes + 6*S);
    double u[3], v[3], eta[3], h[3], gx[3], gy[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        u[i] = swe_ld(ru, k8, i*S8);
        v[i] = swe_ld(rv, k8, i*S8);
        eta[i] = swe_ld(re, k8, i*S8);
        h[i] = swe_ld(rh, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
        gx[i] = swe_ld(rgx, k8, i*S8);
        gy[i] = swe_ld(rgy, k8, i*S8);
    }
    const double A = swe_ld(ra, k8, 0u);
    const double hx = (h[0]*gx[0] + h[1]*gx[1]) + h[2]*gx[2], hy = (h[0]*gy[0] + h[1]*gy[1]) + h[2]*gy[2];
    const double ex = a.nonlinear ? (eta[0]*gx[0] + eta[1]*gx[1]) + eta[2]*gx[2] : 0.0;
    const double ey = a.nonlinear ? (eta[0]*gy[0] + eta[1]*gy[1]) + eta[2]*gy[2] : 0.0;
    double qx[3], qy[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double H = a.nonlinear ? eta[i] + h[i] : h[i];
        double unorm, qfc, mu;
        swe_sediment_friction(a.par.ks, a.par.ksp, a.par.kappa, u[i], v[i], H, unorm, qfc, mu);
        if (COEF) {
            double E, D, ceq;
            swe_sediment_erosion(a.sed, unorm, qfc, mu, H, E, D, ceq);
            swe_st(swe_rsrc(a.sed_planes), k8, i*S8, E);
            swe_st(swe_rsrc(a.sed_planes + 3*S), k8, i*S8, D);
            swe_st(swe_rsrc(a.sed_planes + 6*S), k8, i*S8, ceq);
        }
        swe_bedload_transport<MAG, ANG, SEC>(a.par, a.g, u[i], v[i], H, unorm, qfc, mu, hx, hy, ex, ey, qx[i], qy[i]);
    }
    const double mx = ((qx[0] + qx[1]) + qx[2])/3.0, my = ((qy[0] + qy[1]) + qy[2])/3.0;
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = -(A*(mx*gx[i] + my*gy[i]));
#pragma unroll
    for (int f = 0; f < 3; f++) {
        const int code = swe_ldi(rn, k4, f*S4);
        const unsigned slot = 0u - (unsigned)code;
        const bool open = code < 0 && slot < 32u && ((a.par.open_markers >> (slot & 31u)) & 1u);
        const int b = (f + 1) % 3, o = (f + 2) % 3;
        const double Nx = -((2.0*A)*gx[o]), Ny = -((2.0*A)*gy[o]);
        const double ta = ((2.0*qx[f] + qx[b])*Nx + (2.0*qy[f] + qy[b])*Ny)/6.0;
        const double tb = ((2.0*qx[b] + qx[f])*Nx + (2.0*qy[b] + qy[f])*Ny)/6.0;
        c[f] = open ? c[f] + ta : c[f];
        c[b] = open ? c[b] + tb : c[b];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        swe_st(ox, k8, i*S8, qx[i]);
        swe_st(oy, k8, i*S8, qy[i]);
        swe_st(oc, k8, i*S8, c[i]);
    }
}

struct SweSlideArgs {
    const int *cv;
    const double *vh;
    const double *grad;                         // d psi/dx [3][S] | d psi/dy [3][S]
    const double *area;
    const double *region;                       // [n_cells] or null
    double *planes;                             // alpha [S] | beta [S] | contribution [3][S]
    unsigned long long *words;                  // [0] bits of the largest beta, [1] flagged cells
    size_t stride;
    int n_cells;
    double dt;
    swe2d_slide_params par;
};

// beta >= 0, so the bit pattern of the double orders as the unsigned integer does: the maximum is exact whatever the order of arrival.
// Lanes past the last cell take part in the wave's reductions with beta = 0 and no flag; they load and store nothing.
__global__ void __launch_bounds__(256) swe_slide_kernel(SweSlideArgs a)
{
#pragma clang fp contract(off)
    const int k = blockIdx.x*256 + threadIdx.x;
    const bool in = k < a.n_cells;
    const size_t S = a.stride;
    const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u, S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    double beta = 0.0;
    bool flag = false;
    if (in) {
        const swe_rsrc_t rc = swe_rsrc(a.cv), rh = swe_rsrc(a.vh), rgx = swe_rsrc(a.grad), rgy = swe_rsrc(a.grad + 3*S), ra = swe_rsrc(a.area);
        const swe_rsrc_t oa = swe_rsrc(a.planes), ob = swe_rsrc(a.planes + S), oc = swe_rsrc(a.planes + 2*S);
        double b[3], gx[3], gy[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            b[i] = swe_ld(rh, (unsigned)swe_ldi(rc, k4, i*S4)*8u, 0u);
            gx[i] = swe_ld(rgx, k8, i*S8);
            gy[i] = swe_ld(rgy, k8, i*S8);
        }
        const double A = swe_ld(ra, k8, 0u);
        const double r = a.region ? swe_ld(swe_rsrc(a.region), k8, 0u) : 1.0;
        const double bx = (b[0]*gx[0] + b[1]*gx[1]) + b[2]*gx[2], by = (b[0]*gy[0] + b[1]*gy[1]) + b[2]*gy[2];
        const double sx = r*bx, sy = r*by;
        const double s2 = sx*sx + sy*sy;
        const double nz = 1.0/sqrt(1.0 + s2);
        const double sinb = sqrt(1.0 - nz*nz);
        const double tanbeta = sinb/nz;
        beta = asin(sinb);
        const double d = tanbeta - a.par.tanphi;
        const bool slides = d > 0.0;
        const double L = a.par.length_scale;
        const double cs = slides ? cos(beta*a.dt*a.par.morfac) : 1.0;
        const double qaval = slides ? ((1.0 - a.par.porosity)*0.5*(L*L)*d)/cs : 0.0;
        const bool steep = sinb > 0.0;
        const double q = -(qaval*(nz*nz))/(steep ? sinb : 1.0);
        const double alpha = steep ? q : 0.0;
        double gmax = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double g2 = gx[i]*gx[i] + gy[i]*gy[i];
            gmax = g2 > gmax ? g2 : gmax;
            swe_st(oc, k8, i*S8, (A*alpha)*(gx[i]*bx + gy[i]*by));
        }
        swe_st(oa, k8, 0u, alpha);
        swe_st(ob, k8, 0u, beta);
        flag = alpha > 0.0 || ((a.dt*__builtin_fabs(alpha))*3.0)*gmax > 1.0;
    }
    // the wave's maximum and its number of flagged cells, then at most one atomic each from its first lane
    unsigned long long bits = __builtin_bit_cast(unsigned long long, beta);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(bits, off, 64);
        bits = o > bits ? o : bits;
    }
    const unsigned long long votes = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u) {
        if (bits > __hip_atomic_load(&a.words[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.words[0], bits);
        if (votes) atomicAdd(&a.words[1], (unsigned long long)__popcll(votes));
    }
}

// SED: the net erosion of the sediment field; BED: the bedload contribution planes (a.contrib); SLIDE: the slide's (a.slide), summed
// on their own and scaled by dt alone.  <true, false, false>, <true, true, false> and <false, true, false> are the updates of a handle
// without slide, operation by operation what they were before there was one.
template <bool SED, bool BED, bool SLIDE>
__global__ void __launch_bounds__(256) swe_exner_kernel(SweSedArgs a)
{
#pragma clang fp contract(off)
    const int v = blockIdx.x*256 + threadIdx.x;
    if (v >= a.end) return;
    const size_t S = a.stride;
    const unsigned S8 = (unsigned)S*8u, S4 = (unsigned)S*4u;
    const swe_rsrc_t rb = swe_rsrc(a.contrib), rs = swe_rsrc(a.slide);
    const swe_rsrc_t rE = swe_rsrc(a.planes), rD = swe_rsrc(a.planes + 3*S), re = swe_rsrc(a.state + 6*S), rc = swe_rsrc(a.cv),
                     rh = swe_rsrc(a.vh), rt = swe_rsrc(a.tin), rl = swe_rsrc(a.list), rn = swe_rsrc(a.ent), ra = swe_rsrc(a.area);
    const int e0 = swe_ldi(rl, (unsigned)v*4u, 0u), e1 = swe_ldi(rl, (unsigned)v*4u, 4u);
    const double b_old = swe_ld(rh, (unsigned)v*8u, 0u);
    double num = 0.0, nb = 0.0, ns = 0.0, den = 0.0, eta_min = 1e300;
    for (int e = e0; e < e1; e++) {
        const int ent = swe_ldi(rn, (unsigned)e*4u, 0u);
        const int k = ent >> 2, i = ent & 3;
        const unsigned k8 = (unsigned)k*8u, k4 = (unsigned)k*4u;
        double r[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; SED && j < 3; j++) {
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
        if (SED) num = num + (A/12.0)*((2.0*ri + rj) + rk);
        if (BED) nb = nb + swe_ld(rb, k8, (unsigned)i*S8);
        if (SLIDE) ns = ns + swe_ld(rs, k8, (unsigned)i*S8);
        den = den + A/3.0;
        const double eta = swe_ld(re, k8, (unsigned)i*S8);
        eta_min = eta < eta_min ? eta : eta_min;
    }
    double b_new = b_old;
    if (e1 > e0) {
        const double b = SLIDE ? b_old + (a.dtf*(num + nb) + a.dt*ns)/den
                               : (BED ? b_old + (a.dtf*(num + nb))/den : b_old + (a.dtf*num)/den);
        // the shallowest depth the DG elevation gives at this vertex on the new bed (linear equations: the bed itself)
        const double Hmin = a.nonlinear ? eta_min + b : b;
        if (Hmin >= a.min_depth) b_new = b;
        else atomicAdd(a.count, 1u);
    }
    swe_st(swe_rsrc(a.out), (unsigned)v*8u, 0u, b_new);
}

namespace {

int bedload_launch(Handle *h, bool with_coefficients);

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

// after a model was switched off: the shared tables go with the last model that reads them
void exner_release_unused(Handle *h)
{
    if (!h->sed.on && !h->bed.on && !h->slide.on) h->exner = Handle::Exner();
    if (!h->bed.on && !h->slide.on) h->exner_grad.reset();
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

// the Exner tables (vertex lists, areas, the second bed array, the counter), shared by the sediment field, the bedload model and
// the slide: built aside and moved into place whole
int exner_tables_build(Handle *h)
{
    const int n = h->n_cells, nv = h->n_vertices;
    if (!h->exner.count) {
        Handle::Exner s;
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
        HIP_TRY(h, s.v_off.alloc(off.size()));
        HIP_TRY(h, s.v_ent.alloc(ent.size()));
        HIP_TRY(h, s.area.alloc(n));
        HIP_TRY(h, s.vh_new.alloc(nv));
        HIP_TRY(h, hipMemcpy(s.v_off, off.data(), off.size()*sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(s.v_ent, ent.data(), ent.size()*sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(s.area, area.data(), (size_t)n*sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(h, s.count.alloc(1));
        HIP_TRY(h, hipMemset(s.count, 0, sizeof(unsigned)));
        h->exner = std::move(s);
    }
    return SWE2D_OK;
}

// the three hat-function gradients of every triangle as HostSediment forms them (include/swe2d.h), no contraction: [6][stride]
void bedload_gradients(const Handle *h, const double *vx, const double *vy, std::vector<double> &grad)
{
#pragma clang fp contract(off)
    const int n = h->n_cells;
    const size_t S = h->stride;
    grad.assign(6*S, 0.0);
    for (int k = 0; k < n; k++) {
        const int *c = &h->host_cells[(size_t)3*k];
        const double x0 = vx[c[0]], x1 = vx[c[1]], x2 = vx[c[2]], y0 = vy[c[0]], y1 = vy[c[1]], y2 = vy[c[2]];
        const double p = (x1 - x0)*(y2 - y0), q = (x2 - x0)*(y1 - y0);
        const double det = p - q;
        grad[0*S + k] = (y1 - y2)/det; grad[1*S + k] = (y2 - y0)/det; grad[2*S + k] = (y0 - y1)/det;
        grad[3*S + k] = (x2 - x1)/det; grad[4*S + k] = (x0 - x2)/det; grad[5*S + k] = (x1 - x0)/det;
    }
}

// the gradient table of the bedload pass and the slide, built by whichever comes first
int gradient_table_build(Handle *h)
{
    if (h->exner_grad) return SWE2D_OK;
    const size_t S = h->stride;
    const int nv = h->n_vertices;
    std::vector<double> vx(nv), vy(nv), grad;
    HIP_TRY(h, hipMemcpy(vx.data(), h->vx, (size_t)nv*sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(vy.data(), h->vy, (size_t)nv*sizeof(double), hipMemcpyDeviceToHost));
    bedload_gradients(h, vx.data(), vy.data(), grad);
    DevArray<double> g;
    HIP_TRY(h, g.alloc(6*S));
    HIP_TRY(h, hipMemcpy(g, grad.data(), 6*S*sizeof(double), hipMemcpyHostToDevice));
    h->exner_grad = std::move(g);
    return SWE2D_OK;
}

int exner_check(Handle *h, const char *who)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->sed.on && !h->bed.on && !h->slide.on)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle has neither a sediment model (swe2d_sediment_set) nor a bedload model (swe2d_bedload_set) nor a slide (swe2d_slide_set)");
    return SWE2D_OK;
}

int slide_check(Handle *h, const char *who)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->slide.on) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle has no sediment slide (swe2d_slide_set)");
    return SWE2D_OK;
}

int bedload_check(Handle *h, const char *who)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->bed.on) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle has no bedload model (swe2d_bedload_set)");
    return SWE2D_OK;
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
    if (bedload_fused(h)) {
        if (int rc = bedload_launch(h, true)) return rc;
    } else {
        SWE_CHK_SYNC(h->stream);
        hipLaunchKernelGGL(swe_sediment_coeff_kernel, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, a);
        HIP_TRY(h, hipGetLastError());
    }
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
    const Handle::Exner &x = h->exner;
    SweSedArgs a{};
    sediment_fill(h, a);
    a.tin = s.on ? h->tracers[s.tracer].buf[0].get() : nullptr;
    a.list = x.v_off; a.ent = x.v_ent; a.area = x.area;
    a.out = x.vh_new;
    a.count = x.count;
    a.begin = 0; a.end = h->n_vertices;
    // (a handle without a sediment field takes the factor and the floor from the bedload parameters, one with the slide alone from its)
    a.dtf = h->par.dt*(s.on ? s.par.fac : (h->bed.on ? h->bed.par.fac : h->slide.par.fac));
    a.min_depth = s.on ? s.par.min_depth : (h->bed.on ? h->bed.par.min_depth : h->slide.par.min_depth);
    a.contrib = h->bed.on ? h->bed.planes + 6*h->stride : nullptr;
    a.slide = h->slide.on ? h->slide.planes + 2*h->stride : nullptr;
    a.dt = h->par.dt;
    SWE_CHK_SYNC(h->stream);
    const dim3 grid(grid_for(h->n_vertices)), block(256);
    switch ((s.on ? 1 : 0) | (h->bed.on ? 2 : 0) | (h->slide.on ? 4 : 0)) {
    case 1: hipLaunchKernelGGL((swe_exner_kernel<true, false, false>), grid, block, 0, h->stream, a); break;
    case 2: hipLaunchKernelGGL((swe_exner_kernel<false, true, false>), grid, block, 0, h->stream, a); break;
    case 3: hipLaunchKernelGGL((swe_exner_kernel<true, true, false>), grid, block, 0, h->stream, a); break;
    case 4: hipLaunchKernelGGL((swe_exner_kernel<false, false, true>), grid, block, 0, h->stream, a); break;
    case 5: hipLaunchKernelGGL((swe_exner_kernel<true, false, true>), grid, block, 0, h->stream, a); break;
    case 6: hipLaunchKernelGGL((swe_exner_kernel<false, true, true>), grid, block, 0, h->stream, a); break;
    default: hipLaunchKernelGGL((swe_exner_kernel<true, true, true>), grid, block, 0, h->stream, a); break;
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(h->vh, x.vh_new, (size_t)h->n_vertices*sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return SWE2D_OK;
}

int swe2d_impl::slide_update_launch(Handle *h)
{
    Handle::Slide &sl = h->slide;
    SweSlideArgs a{};
    a.cv = h->cv; a.vh = h->vh;
    a.grad = h->exner_grad; a.area = h->exner.area; a.region = sl.region;
    a.planes = sl.planes; a.words = sl.words;
    a.stride = h->stride;
    a.n_cells = h->n_cells;
    a.dt = h->par.dt;
    a.par = sl.par;
    HIP_TRY(h, hipMemsetAsync(sl.words, 0, sizeof(unsigned long long), h->stream));      // the maximum is that of this pass
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_slide_kernel, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

namespace {
template <bool COEF>
void bedload_dispatch(Handle *h, const SweBedArgs &a)
{
    const swe2d_bedload_params &p = h->bed.par;
    const int sw = (p.use_slope_mag_correction ? 1 : 0) | (p.use_angle_correction ? 2 : 0) | (p.use_secondary_current ? 4 : 0);
    const dim3 grid(grid_for(h->n_cells)), block(256);
    switch (sw) {
    case 0: hipLaunchKernelGGL((swe_bedload_kernel<false, false, false, COEF>), grid, block, 0, h->stream, a); break;
    case 1: hipLaunchKernelGGL((swe_bedload_kernel<true, false, false, COEF>), grid, block, 0, h->stream, a); break;
    case 2: hipLaunchKernelGGL((swe_bedload_kernel<false, true, false, COEF>), grid, block, 0, h->stream, a); break;
    case 3: hipLaunchKernelGGL((swe_bedload_kernel<true, true, false, COEF>), grid, block, 0, h->stream, a); break;
    case 4: hipLaunchKernelGGL((swe_bedload_kernel<false, false, true, COEF>), grid, block, 0, h->stream, a); break;
    case 5: hipLaunchKernelGGL((swe_bedload_kernel<true, false, true, COEF>), grid, block, 0, h->stream, a); break;
    case 6: hipLaunchKernelGGL((swe_bedload_kernel<false, true, true, COEF>), grid, block, 0, h->stream, a); break;
    default: hipLaunchKernelGGL((swe_bedload_kernel<true, true, true, COEF>), grid, block, 0, h->stream, a); break;
    }
}

int bedload_launch(Handle *h, bool with_coefficients)
{
    Handle::Bedload &b = h->bed;
    SweBedArgs a{};
    a.state = h->state[0];
    a.cv = h->cv; a.nbr = h->nbr; a.vh = h->vh;
    a.grad = h->exner_grad; a.area = h->exner.area; a.planes = b.planes;
    a.stride = h->stride;
    a.n_cells = h->n_cells;
    a.nonlinear = h->par.use_nonlinear_equations ? 1 : 0;
    a.g = h->par.g_grav;
    a.par = b.par;
    if (with_coefficients) { a.sed_planes = h->sed.planes; a.sed = h->sed.par; }
    SWE_CHK_SYNC(h->stream);
    if (with_coefficients) bedload_dispatch<true>(h, a);
    else bedload_dispatch<false>(h, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}
}  // namespace

// the sediment update computes q_b in the coefficient pass's launch: asked for (fuse_with_sediment), and the friction closures of
// the two models are the same numbers.  Flow and bed do not change between the sediment update and the bedload pass of a step, so
// the planes are those the separate launch would write.
bool swe2d_impl::bedload_fused(const Handle *h)
{
    const swe2d_bedload_params &b = h->bed.par;
    const swe2d_sediment_params &s = h->sed.par;
    return h->sed.on && h->bed.on && b.fuse_with_sediment && b.ks == s.ks && b.ksp == s.ksp && b.kappa == s.kappa;
}

int swe2d_impl::bedload_update_launch(Handle *h) { return bedload_launch(h, false); }

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
    if (!s.planes) {
        HIP_TRY(h, s.planes.alloc(9*S));
        HIP_TRY(h, hipMemsetAsync(s.planes, 0, 3*plane_bytes, h->stream));
    }
    if (!s.on && (t.source || t.rx.n_code > 0))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_sediment_set: the tracer has a source or a reaction program already (remove it first)");
    if (!t.source) {
        HIP_TRY(h, t.source.alloc(plane_bytes/sizeof(double)));
        HIP_TRY(h, hipMemsetAsync(t.source, 0, plane_bytes, h->stream));
    }
    if (int rc = exner_tables_build(h)) return rc;
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
            HIP_TRY(h, t.bc_value_f.alloc(bytes/sizeof(double)));
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
    t.source.reset();       // (allocated by swe2d_sediment_set: it refuses a tracer with one)
    t.conservative = false;
    h->sed = Handle::Sediment();
    exner_release_unused(h);
    return SWE2D_OK;
}

int swe2d_bedload_set(swe2d_handle *hh, const swe2d_bedload_params *par)
{
    Handle *h = H(hh);
    if (!h || !par) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_bedload_set: null argument");
    if (h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_bedload_set: the sediment model runs on triangles only");
    if (h->n_owned != h->n_cells) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_bedload_set: the sediment model is not available on partitions");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_bedload_set: not with wetting-drying (the depth planes are tied to the bed)");
    if (par->solve_exner && h->n_farms > 0)
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_bedload_set: solve_exner is not available together with tidal turbine farms");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_bedload_set inside a stream capture");
    const double pos[] = {par->thetacr, par->shields_den, par->qb_scale, par->ks, par->ksp, par->kappa, par->rho0, par->fac, par->min_depth};
    for (double x : pos)
        if (!(x > 0.0) || !std::isfinite(x)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_bedload_set: thetacr, shields_den, qb_scale, ks, ksp, kappa, rho0, fac and min_depth must be positive and finite");
    if (!std::isfinite(par->beta) || !(par->surbeta2 >= 0.0) || !std::isfinite(par->surbeta2))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_bedload_set: beta must be finite and surbeta2 >= 0");
    if (par->use_secondary_current && (!(par->alpha_secc > 0.0) || !std::isfinite(par->alpha_secc)))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_bedload_set: alpha_secc must be positive with the secondary current");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Handle::Bedload &b = h->bed;
    const size_t S = h->stride;
    if (int rc = exner_tables_build(h)) return rc;
    if (int rc = gradient_table_build(h)) return rc;
    if (!b.planes) {
        HIP_TRY(h, b.planes.alloc(9*S));
        HIP_TRY(h, hipMemsetAsync(b.planes, 0, 9*S*sizeof(double), h->stream));
    }
    b.par = *par;
    b.on = true;
    return SWE2D_OK;
}

int swe2d_bedload_update(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = bedload_check(h, "swe2d_bedload_update")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return bedload_update_launch(h);
}

int swe2d_bedload_read(swe2d_handle *hh, double *qbx, double *qby, double *contrib)
{
    Handle *h = H(hh);
    if (int rc = bedload_check(h, "swe2d_bedload_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    double *dst[3] = {qbx, qby, contrib};
    for (int q = 0; q < 3; q++) {
        if (!dst[q]) continue;
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                           h->bed.planes + (size_t)3*q*h->stride, h->stage_eta, h->stride, h->n_cells, 3);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(dst[q], h->stage_eta, (size_t)3*h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SWE2D_OK;
}

int swe2d_bedload_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->bed.on) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->bed = Handle::Bedload();
    exner_release_unused(h);
    return SWE2D_OK;
}

int swe2d_slide_set(swe2d_handle *hh, const swe2d_slide_params *par, const double *region_per_cell)
{
    Handle *h = H(hh);
    if (!h || !par) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_slide_set: null argument");
    if (h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_slide_set: the sediment model runs on triangles only");
    if (h->n_owned != h->n_cells) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_slide_set: the sediment model is not available on partitions");
    if (h->wd) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_slide_set: not with wetting-drying (the depth planes are tied to the bed)");
    if (par->solve_exner && h->n_farms > 0)
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_slide_set: solve_exner is not available together with tidal turbine farms");
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_slide_set inside a stream capture");
    const double pos[] = {par->tanphi, par->length_scale, par->morfac, par->fac, par->min_depth};
    for (double x : pos)
        if (!(x > 0.0) || !std::isfinite(x)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_slide_set: tanphi, length_scale, morfac, fac and min_depth must be positive and finite");
    if (!(par->porosity >= 0.0) || !(par->porosity < 1.0))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_slide_set: porosity must lie in [0, 1)");
    if (region_per_cell)
        for (int k = 0; k < h->n_cells; k++)
            if (!std::isfinite(region_per_cell[k])) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_slide_set: the region must be finite");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Handle::Slide &sl = h->slide;
    const size_t S = h->stride;
    if (int rc = exner_tables_build(h)) return rc;
    if (int rc = gradient_table_build(h)) return rc;
    if (!sl.planes) {
        HIP_TRY(h, sl.planes.alloc(5*S));
        HIP_TRY(h, hipMemsetAsync(sl.planes, 0, 5*S*sizeof(double), h->stream));
    }
    HIP_TRY(h, sl.words.ensure(2));
    HIP_TRY(h, hipMemsetAsync(sl.words, 0, 2*sizeof(unsigned long long), h->stream));
    if (region_per_cell) {
        HIP_TRY(h, sl.region.ensure((size_t)h->n_cells));
        HIP_TRY(h, hipMemcpyAsync(sl.region, region_per_cell, (size_t)h->n_cells*sizeof(double), hipMemcpyHostToDevice, h->stream));
    } else {
        sl.region.reset();
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    sl.par = *par;
    sl.on = true;
    return SWE2D_OK;
}

int swe2d_slide_update(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = slide_check(h, "swe2d_slide_update")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return slide_update_launch(h);
}

int swe2d_slide_read(swe2d_handle *hh, double *alpha, double *beta, double *contrib)
{
    Handle *h = H(hh);
    if (int rc = slide_check(h, "swe2d_slide_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t S = h->stride;
    double *cell[2] = {alpha, beta};
    for (int q = 0; q < 2; q++)
        if (cell[q]) HIP_TRY(h, hipMemcpyAsync(cell[q], h->slide.planes + q*S, (size_t)h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (contrib) {
        hipLaunchKernelGGL(swe_planes_to_nodal, dim3(grid_for(h->n_cells)), dim3(256), 0, h->stream,
                           h->slide.planes + 2*S, h->stage_eta, h->stride, h->n_cells, 3);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(contrib, h->stage_eta, (size_t)3*h->n_cells*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

int swe2d_slide_max_angle(swe2d_handle *hh, double *beta_max)
{
    Handle *h = H(hh);
    if (int rc = slide_check(h, "swe2d_slide_max_angle")) return rc;
    if (!beta_max) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long bits = 0;
    HIP_TRY(h, hipMemcpyAsync(&bits, h->slide.words, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::memcpy(beta_max, &bits, sizeof(double));
    return SWE2D_OK;
}

int swe2d_slide_flagged(swe2d_handle *hh, int64_t *n_flagged)
{
    Handle *h = H(hh);
    if (int rc = slide_check(h, "swe2d_slide_flagged")) return rc;
    if (!n_flagged) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long c = 0;
    HIP_TRY(h, hipMemcpyAsync(&c, h->slide.words + 1, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_flagged = (int64_t)c;
    return SWE2D_OK;
}

int swe2d_slide_clear(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (!h->slide.on) return SWE2D_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->slide = Handle::Slide();
    exner_release_unused(h);
    return SWE2D_OK;
}

int swe2d_exner_step(swe2d_handle *hh)
{
    Handle *h = H(hh);
    if (int rc = exner_check(h, "swe2d_exner_step")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return exner_launch(h);
}

int swe2d_exner_skipped(swe2d_handle *hh, int64_t *n_skipped)
{
    Handle *h = H(hh);
    if (int rc = exner_check(h, "swe2d_exner_skipped")) return rc;
    if (!n_skipped) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned c = 0;
    HIP_TRY(h, hipMemcpyAsync(&c, h->exner.count, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
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
