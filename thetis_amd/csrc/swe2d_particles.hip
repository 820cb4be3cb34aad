// swe2d_particles.hip - Lagrangian particle tracking: the swe2d_particles_* entry points and the advection kernel.
//
// A particle set holds, per particle, its position [n][2], its cell, status, exit marker and wall-hit counter (four int planes [n]),
// and `capacity` rows [n][2] of recorded positions.  swe_particle_kernel - one lane per particle - makes one explicit-midpoint move in
// the velocity planes of buffer A, frozen over the move:
//
//     u1 = U(x, k);   (xm, km) = probe(x, k, (0.5*dt_move)*u1);   u2 = U(xm, km);   (x', k') = move(x, k, dt_move*u2)
//
// with U the P1 interpolation of the cell's nodal velocities and move() the straight walk from cell to cell through the packed
// neighbour codes (include/swe2d.h has the formulas, thetis_amd/particles.py restates them in numpy).  Everything is evaluated left
// to right without contraction and uses + - * / and comparisons only, so a host replay has the bits of the device.  The walk is a
// divergent gather by nature: per cell visited a lane reads 3 vertex ids, 6 vertex coordinates and 1 neighbour code (64 B), per
// velocity 6 nodal values and the cell's geometry (108 B); per advance 16 B of position and 8 B of cell / status are read, 16 + 4 B
// written (more on an exit or a wall hit).  No LDS, no atomics, every particle has exactly one writer.  The plane pointers are taken
// from the handle when the launch is enqueued, so an advance after a launch that swapped the state buffers (swe_fuse123_kernel)
// sees the step result, as a probe row does.
//
// Opt-in per set (include/swe2d.h has the formulas): swe2d_particles_advance_at launches swe_particle_walk_kernel<TIMED, WALK>, the
// same lane body with a release gate in front (TIMED: a WAITING particle whose time has come turns ACTIVE) and Visser's random walk
// behind the midpoint move (WALK: the diffusivity of the cell's three vertices, ten Philox rounds on the counter (particle, move),
// one IEEE square root and a second walk).  swe_particle_kernel is the <false, false> body: a set without either runs the
// instructions it ran before these existed.  swe2d_particles_cell_counts is one launch of 32-bit integer atomic adds.
#include "swe2d_handle.h"

#ifndef SWE_RANGE_CHECK
__device__ __forceinline__ void swe_sti(swe_rsrc_t r, unsigned voff, unsigned soff, int x)
{
    __builtin_amdgcn_raw_buffer_store_b32((unsigned)x, r, voff, soff, 0);
}
#else
__device__ __forceinline__ void swe_sti_chk(swe_rsrc_t r, unsigned voff, unsigned soff, int x, int line)
{
    if (!swe_chk(r.base + voff + soff, 4, line)) return;
    __builtin_amdgcn_raw_buffer_store_b32((unsigned)x, r.r, voff, soff, 0);
}
#define swe_sti(r, v, s, x) swe_sti_chk(r, v, s, x, __LINE__)
#endif

struct SweParticleArgs {
    const double *state;                        // buffer A: u planes | v planes | elevation planes, [9][stride]
    const int *cv, *nbr;                        // [3][stride] cell vertices, packed neighbour codes
    const double *vx, *vy;                      // vertex coordinates
    double *pos;                                // [n][2]
    int *ist;                                   // cell [n] | status [n] | exit marker [n] | wall hits [n]
    size_t stride;
    double dt_move;
    int n;
    unsigned open_mask;                         // bit m: boundary marker m is open
};

struct SweParticleCell { double x0, y0, ax, ay, bx, by, det; };

enum { SWE_WALK_ARRIVED = 0, SWE_WALK_EXIT = 1, SWE_WALK_WALL = 2, SWE_WALK_LOST = 3 };

__device__ __forceinline__ SweParticleCell swe_particle_cell(const SweParticleArgs &a, int k)
{
#pragma clang fp contract(off)
    const unsigned k4 = (unsigned)k*4u, S4 = (unsigned)a.stride*4u;
    const swe_rsrc_t rc = swe_rsrc(a.cv), rx = swe_rsrc(a.vx), ry = swe_rsrc(a.vy);
    const unsigned v0 = (unsigned)swe_ldi(rc, k4, 0u)*8u, v1 = (unsigned)swe_ldi(rc, k4, S4)*8u, v2 = (unsigned)swe_ldi(rc, k4, 2u*S4)*8u;
    SweParticleCell c;
    c.x0 = swe_ld(rx, v0, 0u);
    c.y0 = swe_ld(ry, v0, 0u);
    c.ax = swe_ld(rx, v1, 0u) - c.x0;
    c.ay = swe_ld(ry, v1, 0u) - c.y0;
    c.bx = swe_ld(rx, v2, 0u) - c.x0;
    c.by = swe_ld(ry, v2, 0u) - c.y0;
    c.det = c.ax*c.by - c.bx*c.ay;
    return c;
}

// m[f]: the barycentric coordinate that vanishes on facet f (the one of the local vertex (f + 2) % 3)
__device__ __forceinline__ void swe_particle_bary(const SweParticleCell &c, double px, double py, double m[3])
{
#pragma clang fp contract(off)
    const double dx = px - c.x0, dy = py - c.y0;
    const double l1 = (dx*c.by - c.bx*dy)/c.det;
    const double l2 = (c.ax*dy - dx*c.ay)/c.det;
    const double l0 = (1.0 - l1) - l2;
    m[0] = l2; m[1] = l0; m[2] = l1;
}

__device__ __forceinline__ void swe_particle_velocity(const SweParticleArgs &a, int k, double px, double py, double &u, double &v)
{
#pragma clang fp contract(off)
    const SweParticleCell c = swe_particle_cell(a, k);
    double m[3];
    swe_particle_bary(c, px, py, m);
    const unsigned k8 = (unsigned)k*8u, S8 = (unsigned)a.stride*8u;
    const swe_rsrc_t gu = swe_rsrc(a.state), gv = swe_rsrc(a.state + 3*a.stride);
    const double u0 = swe_ld(gu, k8, 0u), u1 = swe_ld(gu, k8, S8), u2 = swe_ld(gu, k8, 2u*S8);
    const double v0 = swe_ld(gv, k8, 0u), v1 = swe_ld(gv, k8, S8), v2 = swe_ld(gv, k8, 2u*S8);
    u = (m[1]*u0 + m[2]*u1) + m[0]*u2;
    v = (m[1]*v0 + m[2]*v1) + m[0]*v2;
}

// the straight walk along (x, y) -> (x + dx, y + dy) from cell k: where it ends (ox, oy, ok), how, and through which marker
__device__ __forceinline__ int swe_particle_walk(const SweParticleArgs &a, double x, double y, int k, double dx, double dy,
                                                 double &ox, double &oy, int &ok, int &marker)
{
#pragma clang fp contract(off)
    const double tx = x + dx, ty = y + dy;
    const unsigned S4 = (unsigned)a.stride*4u;
    const swe_rsrc_t rn = swe_rsrc(a.nbr);
    int from = -1;
    for (int hop = 0; hop < SWE2D_PARTICLE_MAX_HOPS; hop++) {          // bounded: no lane loops forever
        const SweParticleCell c = swe_particle_cell(a, k);
        double mx[3], my[3];
        swe_particle_bary(c, x, y, mx);
        swe_particle_bary(c, tx, ty, my);
        int best = -1;
        double sb = 0.0;
#pragma unroll
        for (int f = 0; f < 3; f++) {
            if (f != from && my[f] < 0.0) {
                const double s = mx[f]/(mx[f] - my[f]);
                if (best < 0 || s < sb) { best = f; sb = s; }
            }
        }
        if (best < 0) { ox = tx; oy = ty; ok = k; return SWE_WALK_ARRIVED; }
        const int code = swe_ldi(rn, (unsigned)k*4u + (unsigned)best*S4, 0u);
        if (code >= 0) { from = code & 3; k = code >> 2; continue; }
        marker = -code;
        ok = k;
        if (marker < SWE2D_MAX_MARKERS && ((a.open_mask >> marker) & 1u)) {
            ox = x + sb*dx; oy = y + sb*dy;
            return SWE_WALK_EXIT;
        }
        const double f = sb*(1.0 - 0x1p-10);
        ox = x + f*dx; oy = y + f*dy;
        return SWE_WALK_WALL;
    }
    return SWE_WALK_LOST;
}

// what the opt-in instances read on top of SweParticleArgs: the release gate (TIMED) and the random walk (WALK)
struct SweParticleExtra {
    const double *release;                      // [n] release times (TIMED)
    const double *kv;                           // [n_vertices] diffusivity at the vertices (WALK)
    double t;                                   // the time at which the move ends (TIMED)
    unsigned key0, key1;                        // the low and the high half of the seed (WALK)
    unsigned move;                              // moves the set has made before this one (WALK)
};

// Philox4x32-10 (Salmon et al. 2011): ten rounds on the counter c under the key (k0, k1), which goes up by the Weyl constants between rounds
__device__ __forceinline__ void swe_philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u*c[0];
        const unsigned h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u*c[2];
        const unsigned n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// a deviate on [-1, 1) from 27 + 26 bits of two words: every operation is exact in doubles
__device__ __forceinline__ double swe_particle_deviate(unsigned wa, unsigned wb)
{
#pragma clang fp contract(off)
    return 2.0*(((double)(wa >> 5)*67108864.0 + (double)(wb >> 6))*0x1p-53) - 1.0;
}

// Visser's (1997) random-walk displacement of particle p at (x, y) in cell k: dt*grad K + sqrt(6 dt K(offset))*R
__device__ __forceinline__ void swe_particle_dispersion(const SweParticleArgs &a, const SweParticleExtra &e, int p, int k, double x, double y,
                                                        double &dx, double &dy)
{
#pragma clang fp contract(off)
    const SweParticleCell c = swe_particle_cell(a, k);
    double m[3];
    swe_particle_bary(c, x, y, m);
    const unsigned k4 = (unsigned)k*4u, S4 = (unsigned)a.stride*4u;
    const swe_rsrc_t rc = swe_rsrc(a.cv), rk = swe_rsrc(e.kv);
    const double K0 = swe_ld(rk, (unsigned)swe_ldi(rc, k4, 0u)*8u, 0u), K1 = swe_ld(rk, (unsigned)swe_ldi(rc, k4, S4)*8u, 0u),
                 K2 = swe_ld(rk, (unsigned)swe_ldi(rc, k4, 2u*S4)*8u, 0u);
    const double Kx = (m[1]*K0 + m[2]*K1) + m[0]*K2;
    const double gx = ((K1 - K0)*c.by - (K2 - K0)*c.ay)/c.det;
    const double gy = (c.ax*(K2 - K0) - c.bx*(K1 - K0))/c.det;
    double Ko = Kx + (0.5*a.dt_move)*(gx*gx + gy*gy);
    if (Ko < 0.0) Ko = 0.0;
    const double amp = sqrt((6.0*a.dt_move)*Ko);            // the correctly rounded IEEE square root, as numpy's
    unsigned w[4] = {(unsigned)p, e.move, 0u, 0u};
    swe_philox4x32_10(w, e.key0, e.key1);
    dx = a.dt_move*gx + amp*swe_particle_deviate(w[0], w[1]);
    dy = a.dt_move*gy + amp*swe_particle_deviate(w[2], w[3]);
}

// One move of particle p.  TIMED: a WAITING particle whose release time has come turns ACTIVE first.  WALK: the random-walk step
// follows the midpoint move that arrived or ended at a wall.  <false, false> is the move of a set without either.
template <bool TIMED, bool WALK>
__device__ __forceinline__ void swe_particle_move(const SweParticleArgs &a, const SweParticleExtra &e, int p)
{
#pragma clang fp contract(off)
    const swe_rsrc_t ri = swe_rsrc(a.ist), rp = swe_rsrc(a.pos);
    const unsigned p4 = (unsigned)p*4u, p16 = (unsigned)p*16u, N4 = (unsigned)a.n*4u;
    const int status = swe_ldi(ri, p4, N4);
    if (TIMED && status == SWE2D_PARTICLE_WAITING) {
        if (!(e.t - a.dt_move >= swe_ld(swe_rsrc(e.release), (unsigned)p*8u, 0u))) return;
        swe_sti(ri, p4, N4, SWE2D_PARTICLE_ACTIVE);
    } else if (status != SWE2D_PARTICLE_ACTIVE) {
        return;
    }
    const int k = swe_ldi(ri, p4, 0u);
    const double x = swe_ld(rp, p16, 0u), y = swe_ld(rp, p16, 8u);
    double u, v, xm, ym, xn, yn;
    int km, kn, marker = 0;
    swe_particle_velocity(a, k, x, y, u, v);
    const double half = 0.5*a.dt_move;
    int how = swe_particle_walk(a, x, y, k, half*u, half*v, xm, ym, km, marker);
    if (how != SWE_WALK_LOST) {
        swe_particle_velocity(a, km, xm, ym, u, v);
        how = swe_particle_walk(a, x, y, k, a.dt_move*u, a.dt_move*v, xn, yn, kn, marker);
    }
    int hits = how == SWE_WALK_WALL ? 1 : 0;
    if (WALK && (how == SWE_WALK_ARRIVED || how == SWE_WALK_WALL)) {
        double dx, dy;
        swe_particle_dispersion(a, e, p, kn, xn, yn, dx, dy);
        if (dx != 0.0 || dy != 0.0) {                       // (a zero displacement is no walk: the particle stays where it is)
            const double xa = xn, ya = yn;
            const int ka = kn;
            how = swe_particle_walk(a, xa, ya, ka, dx, dy, xn, yn, kn, marker);
            if (how == SWE_WALK_WALL) hits++;
        }
    }
    if (how == SWE_WALK_LOST) {
        swe_sti(ri, p4, N4, SWE2D_PARTICLE_LOST);
        return;
    }
    swe_st(rp, p16, 0u, xn);
    swe_st(rp, p16, 8u, yn);
    swe_sti(ri, p4, 0u, kn);
    if (how == SWE_WALK_EXIT) {
        swe_sti(ri, p4, N4, SWE2D_PARTICLE_EXITED);
        swe_sti(ri, p4, 2u*N4, marker);
    } else if (!WALK && how == SWE_WALK_WALL) {
        swe_sti(ri, p4, 3u*N4, swe_ldi(ri, p4, 3u*N4) + 1);
    }
    if (WALK && hits > 0) swe_sti(ri, p4, 3u*N4, swe_ldi(ri, p4, 3u*N4) + hits);    // (the midpoint move's wall and the walk's own)
}

__global__ void __launch_bounds__(256) swe_particle_kernel(SweParticleArgs a)
{
    const int p = blockIdx.x*blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    swe_particle_move<false, false>(a, SweParticleExtra{}, p);
}

// the opt-in instances: timed releases, the random walk, both
template <bool TIMED, bool WALK>
__global__ void __launch_bounds__(256) swe_particle_walk_kernel(SweParticleArgs a, SweParticleExtra e)
{
    const int p = blockIdx.x*blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    swe_particle_move<TIMED, WALK>(a, e, p);
}

// counts[cell] += 1 for every particle whose status is in the mask: integer atomics, so the order does not matter
__global__ void __launch_bounds__(256) swe_particle_count_kernel(const int *ist, int n, unsigned status_mask, int n_cells, int *counts)
{
    const int p = blockIdx.x*blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int k = ist[p], status = ist[(size_t)n + p];
    if ((unsigned)status < 32u && ((status_mask >> status) & 1u) && (unsigned)k < (unsigned)n_cells) atomicAdd(&counts[k], 1);
}

namespace {

const int kParticlesMax = 1 << 27;              // 16 B of position per particle behind a 32-bit offset

int particles_check(Handle *h, int id, Handle::Particles **out)
{
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "particle calls are not allowed inside a stream capture");
    if (id < 0 || id >= (int)h->particles.size() || !h->particles[id].live)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "no such particle set");
    *out = &h->particles[id];
    return SWE2D_OK;
}

// the bit mask of the open markers of an advance, or false (the handle has the message)
bool particles_open_mask(Handle *h, int n_open, const int32_t *open_markers, double dt_move, const char *who, unsigned *mask)
{
    if (n_open < 0 || n_open > SWE2D_MAX_MARKERS || (n_open > 0 && !open_markers) || !std::isfinite(dt_move)) {
        fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": bad argument");
        return false;
    }
    *mask = 0u;
    for (int j = 0; j < n_open; j++) {
        if (open_markers[j] < 1 || open_markers[j] >= SWE2D_MAX_MARKERS) {
            fail(h, SWE2D_ERR_INVALID_ARGUMENT, std::string(who) + ": open markers must be in 1..SWE2D_MAX_MARKERS-1");
            return false;
        }
        *mask |= 1u << open_markers[j];
    }
    return true;
}

SweParticleArgs particles_args(const Handle *h, const Handle::Particles *s, double dt_move, unsigned mask)
{
    SweParticleArgs a{};
    a.state = h->state[0];
    a.cv = h->cv; a.nbr = h->nbr; a.vx = h->vx; a.vy = h->vy;
    a.pos = s->pos; a.ist = s->ist;
    a.stride = h->stride;
    a.dt_move = dt_move;
    a.n = s->n;
    a.open_mask = mask;
    return a;
}

}  // namespace

int swe2d_particles_create(swe2d_handle *hh, int32_t n, const double *xy, const int32_t *cells, int32_t capacity, int32_t *particles_id)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (stream_capturing(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "particle calls are not allowed inside a stream capture");
    if (h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_particles_create: particles are tracked on triangles only");
    if (n <= 0 || n > kParticlesMax || !xy || !cells || capacity < 0 || !particles_id)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_create: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    {   // every cell in range, every position inside its cell: the formulas of the kernel on the host's copy of the vertices
        std::vector<double> vx((size_t)h->n_vertices), vy((size_t)h->n_vertices);
        HIP_TRY(h, hipMemcpy(vx.data(), h->vx, vx.size()*sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(vy.data(), h->vy, vy.size()*sizeof(double), hipMemcpyDeviceToHost));
        for (int p = 0; p < n; p++) {
            const int k = cells[p];
            if (k < 0 || k >= h->n_cells) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_create: cell out of range");
            const int *v = &h->host_cells[(size_t)3*k];
            const double x0 = vx[v[0]], y0 = vy[v[0]], ax = vx[v[1]] - x0, ay = vy[v[1]] - y0, bx = vx[v[2]] - x0, by = vy[v[2]] - y0;
            const double det = ax*by - bx*ay, dx = xy[2*(size_t)p] - x0, dy = xy[2*(size_t)p + 1] - y0;
            const double l1 = (dx*by - bx*dy)/det, l2 = (ax*dy - dx*ay)/det, l0 = (1.0 - l1) - l2;
            if (!(l0 >= -1e-12 && l1 >= -1e-12 && l2 >= -1e-12))
                return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_create: particle " + std::to_string(p) + " is not inside its cell");
        }
    }
    Handle::Particles s;
    s.n = n; s.capacity = capacity;
    HIP_TRY(h, s.pos.alloc((size_t)n*2));
    HIP_TRY(h, s.ist.alloc((size_t)n*4));
    HIP_TRY(h, s.out.alloc((size_t)std::max(capacity, 1)*n*2));
    HIP_TRY(h, hipMemcpyAsync(s.pos, xy, (size_t)n*2*sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(s.ist, 0, (size_t)n*4*sizeof(int), h->stream));         // ACTIVE, no marker, no hits
    HIP_TRY(h, hipMemcpyAsync(s.ist, cells, (size_t)n*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                                   // the host arrays may be reused by the caller
    s.live = true;
    int id = 0;
    while (id < (int)h->particles.size() && h->particles[id].live) id++;
    if (id == (int)h->particles.size()) h->particles.push_back(std::move(s)); else h->particles[id] = std::move(s);
    *particles_id = id;
    return SWE2D_OK;
}

int swe2d_particles_advance(swe2d_handle *hh, int32_t id, double dt_move, int32_t n_open, const int32_t *open_markers)
{
    Handle *h = H(hh);
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    unsigned mask = 0u;
    if (!particles_open_mask(h, n_open, open_markers, dt_move, "swe2d_particles_advance", &mask)) return SWE2D_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    const SweParticleArgs a = particles_args(h, s, dt_move, mask);
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(swe_particle_kernel, dim3((unsigned)grid_for(s->n)), dim3(256), 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    return SWE2D_OK;
}

int swe2d_particles_set_diffusivity(swe2d_handle *hh, int32_t id, int32_t n_vertices, const double *diffusivity, uint64_t seed)
{
    Handle *h = H(hh);
    if (h && h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_particles_set_diffusivity: particles are tracked on triangles only");
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    if (n_vertices != h->n_vertices || !diffusivity)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_set_diffusivity: the table has one value per vertex of the mesh");
    for (int v = 0; v < n_vertices; v++)
        if (!(diffusivity[v] >= 0.0) || !std::isfinite(diffusivity[v]))
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_set_diffusivity: the diffusivity must be finite and not negative");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)n_vertices*sizeof(double);
    HIP_TRY(h, s->kv.ensure(n_vertices));
    HIP_TRY(h, hipMemcpyAsync(s->kv, diffusivity, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                           // the host array may be reused by the caller
    s->seed = seed;
    return SWE2D_OK;
}

int swe2d_particles_set_release_times(swe2d_handle *hh, int32_t id, int32_t n, const double *release_times, double t_now)
{
    Handle *h = H(hh);
    if (h && h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_particles_set_release_times: particles are tracked on triangles only");
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    if (n != s->n || !release_times || std::isnan(t_now))
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_set_release_times: one release time per particle");
    for (int p = 0; p < n; p++)
        if (std::isnan(release_times[p]))
            return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_set_release_times: a release time is not a number");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)n*sizeof(double);
    HIP_TRY(h, s->release.ensure(n));
    // ACTIVE <-> WAITING by the new times; EXITED and LOST particles stay what they are
    std::vector<int> status((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(status.data(), s->ist + (size_t)n, (size_t)n*sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int p = 0; p < n; p++)
        if (status[p] == SWE2D_PARTICLE_ACTIVE || status[p] == SWE2D_PARTICLE_WAITING)
            status[p] = release_times[p] > t_now ? SWE2D_PARTICLE_WAITING : SWE2D_PARTICLE_ACTIVE;
    HIP_TRY(h, hipMemcpyAsync(s->release, release_times, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(s->ist + (size_t)n, status.data(), (size_t)n*sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SWE2D_OK;
}

int swe2d_particles_advance_at(swe2d_handle *hh, int32_t id, double dt_move, double t, int32_t n_open, const int32_t *open_markers)
{
    Handle *h = H(hh);
    if (h && h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_particles_advance_at: particles are tracked on triangles only");
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    unsigned mask = 0u;
    if (!particles_open_mask(h, n_open, open_markers, dt_move, "swe2d_particles_advance_at", &mask)) return SWE2D_ERR_INVALID_ARGUMENT;
    if (std::isnan(t)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_advance_at: the time is not a number");
    if (s->kv && dt_move < 0.0)
        return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_advance_at: a random walk cannot go back in time (dt_move < 0)");
    HIP_TRY(h, hipSetDevice(h->device));
    const SweParticleArgs a = particles_args(h, s, dt_move, mask);
    SweParticleExtra e{};
    e.release = s->release; e.kv = s->kv;
    e.t = t;
    e.key0 = (unsigned)(s->seed & 0xffffffffull); e.key1 = (unsigned)(s->seed >> 32);
    e.move = s->moves;
    const dim3 grid((unsigned)grid_for(s->n)), block(256);
    SWE_CHK_SYNC(h->stream);
    if (s->release && s->kv) hipLaunchKernelGGL((swe_particle_walk_kernel<true, true>), grid, block, 0, h->stream, a, e);
    else if (s->kv) hipLaunchKernelGGL((swe_particle_walk_kernel<false, true>), grid, block, 0, h->stream, a, e);
    else if (s->release) hipLaunchKernelGGL((swe_particle_walk_kernel<true, false>), grid, block, 0, h->stream, a, e);
    else hipLaunchKernelGGL(swe_particle_kernel, grid, block, 0, h->stream, a);
    HIP_TRY(h, hipGetLastError());
    s->moves++;
    return SWE2D_OK;
}

int swe2d_particles_cell_counts(swe2d_handle *hh, int32_t id, uint32_t status_mask, int32_t *counts)
{
    Handle *h = H(hh);
    if (h && h->npc != 3) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_particles_cell_counts: particles are tracked on triangles only");
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    if (!counts) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)h->n_cells*sizeof(int);
    HIP_TRY(h, s->counts.ensure(h->n_cells));
    HIP_TRY(h, hipMemsetAsync(s->counts, 0, bytes, h->stream));
    hipLaunchKernelGGL(swe_particle_count_kernel, dim3((unsigned)grid_for(s->n)), dim3(256), 0, h->stream, s->ist, s->n, status_mask,
                       h->n_cells, s->counts);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(counts, s->counts, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = capture_parity_check(h)) return rc;
    return flow_check(h);
}

int swe2d_particles_record(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    if (s->rows >= s->capacity) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "swe2d_particles_record: the row buffer is full (read it first)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t row = (size_t)s->n*2;
    HIP_TRY(h, hipMemcpyAsync(s->out + (size_t)s->rows*row, s->pos, row*sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    s->rows++;
    return SWE2D_OK;
}

int swe2d_particles_read(swe2d_handle *hh, int32_t id, double *xy, int32_t *cells, int32_t *status, int32_t *exit_markers, int32_t *wall_hits)
{
    Handle *h = H(hh);
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)s->n;
    if (xy) HIP_TRY(h, hipMemcpyAsync(xy, s->pos, 2*n*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int32_t *dst[4] = {cells, status, exit_markers, wall_hits};
    for (int j = 0; j < 4; j++)
        if (dst[j]) HIP_TRY(h, hipMemcpyAsync(dst[j], s->ist + (size_t)j*n, n*sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = capture_parity_check(h)) return rc;
    return flow_check(h);
}

int swe2d_particles_read_rows(swe2d_handle *hh, int32_t id, double *out, int32_t *n_rows)
{
    Handle *h = H(hh);
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    if (!out || !n_rows) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    if (s->rows > 0)
        HIP_TRY(h, hipMemcpyAsync(out, s->out, (size_t)s->rows*s->n*2*sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    *n_rows = s->rows;
    s->rows = 0;
    if (int rc = capture_parity_check(h)) return rc;
    return flow_check(h);
}

int swe2d_particles_destroy(swe2d_handle *hh, int32_t id)
{
    Handle *h = H(hh);
    Handle::Particles *s = nullptr;
    if (int rc = particles_check(h, id, &s)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));                           // moves may still be in flight
    *s = Handle::Particles();
    return SWE2D_OK;
}
