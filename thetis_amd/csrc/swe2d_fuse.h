// swe2d_fuse.h - stages 1 and 2 of an SSPRK33 step in ONE launch by overlapped tiles.  What swe2d_advance takes by itself from
// 250 k triangles on a whole mesh the kernel covers (swe2d_plan.hip: step_plan; SWE2D_OPT_FUSED_STAGES forces or forbids it).
//
// A stage launch streams the state: per triangle and step 72 B read + 72 B written in stage 1, 72 + 72 B read + 72 B written in
// stage 2.  U(1) is read by stage 2 and by nothing else (rungekutta.py:ERKGenericShuOsher, stage 3 takes
// U(2) and U(0)), so a workgroup that owns a TILE of the mesh can keep it on chip: 256 lanes = up to 192 interior cells (lanes
// 0 .. n_inner-1: three waves) + the cells that share a facet with them (the ring, at most 64: the fourth wave).  Stage 1 is
// evaluated for every cell of the tile - the ring's redundantly, its outer neighbours' traces gathered from the state planes -,
// the results go to LDS, and stage 2 is evaluated for the interior cells with every neighbour trace from LDS.  Per interior
// cell the launch reads U(0) once (x 1.24 for the ring on the bench mesh) and writes U(2): 192 MB per launch at 1 M cells by the
// counters where the two stage launches move 428 MB.
// The arithmetic of a cell is swe2d_tri.h's, the functions swe_stage_kernel calls (the traces come from LDS: swe_flow_rhs_facets):
// bit for bit the stage launches (tests/test_gpu_parity.py::test_fused_stage_pair_gives_the_bits_...), and checked directly against
// the oracle (::test_fused_stage_pair_matches_the_c_restatement...).
// Covers: triangles, whole mesh or the owned + ghost ranges of a partition, with or without source terms; no wetting-drying, no
// viscosity (those keep the stage launches).
#pragma once
#include "swe2d_kernels.h"
#include "swe2d_flow.h"

#ifndef SWE_FUSE_WG
#define SWE_FUSE_WG 256
#endif
#ifndef SWE_FUSE_MIN_WG
#define SWE_FUSE_MIN_WG 3                                 // workgroups per CU the compiler has to make room for (3: 168 VGPRs)
#endif
#ifndef SWE_FUSE_INNER
#define SWE_FUSE_INNER 192
#endif
#define SWE_FUSE_FBITS 10                                // bits per facet in the tile table's packed word: 9 of lane / slot + the flag
#define SWE_FUSE_RING (SWE_FUSE_WG - SWE_FUSE_INNER)
#define SWE_FUSE_XG (9*SWE_FUSE_WG)                    // staging area of the traces from outside the tile: [slot][6]
#define SWE_FUSE_MAX_OUT (2*SWE_FUSE_RING)             // a ring cell has a facet towards the interior: at most two towards the outside
#define SWE_FUSE_LDS (SWE_FUSE_XG + 6*SWE_FUSE_MAX_OUT)

struct SweFuseArgs {
    SweStageArgs st;          // uin = U(0) (state buffer A); geometry, connectivity, boundary tables; dt, g, sigma_lf
    const int2 *tile;         // [n_tiles][256]: {cell or -1, per facet 10 bits: [8:0] lane of the neighbour in the tile (a boundary
                              //  facet: the lane itself) or, with bit 9 set, the staging slot of a neighbour outside the tile}
    const int *n_inner;       // [n_tiles]: lanes 0 .. n_inner-1 hold the interior cells
    int n_tiles;
    int cell_end;             // stage 2 updates the interior cells < cell_end (a partition's shrinking stage ranges; else n_cells)
    double beta1;             // stage 1: U(1) = U(0) + beta1 dt M^-1 R(U(0))
    double a0_2, a1_2, beta2; // stage 2: U(2) = a0 U(0) + a1 U(1) + beta2 dt M^-1 R(U(1))
    double *out;              // 9 planes: U(2) (state buffer C)
};

template <bool NONLIN, bool LF, bool SRC = false>
__global__ __launch_bounds__(SWE_FUSE_WG, SWE_FUSE_MIN_WG) void swe_fuse12_kernel(const SweFuseArgs q)
{
#pragma clang fp contract(off)
    __shared__ double lds[SWE_FUSE_LDS];
    __shared__ double lw[9][SWE_FUSE_INNER];               // a0 U(0) + a1 U(1) of the interior cells: 18 registers stage 2 cannot spare
    const SweStageArgs &p = q.st;
    const int tile = swe_logical_block(blockIdx.x, gridDim.x);
    if (tile >= q.n_tiles) return;                         // padding of the grid to a multiple of 8
    const int lane = (int)threadIdx.x;
    const int2 tl = q.tile[(size_t)tile*SWE_FUSE_WG + lane];
    const bool real = tl.x >= 0;
    const int k = real ? tl.x : 0;
    const int n_inner = q.n_inner[tile];
    const size_t S = p.stride;
    const unsigned S8 = (unsigned)S*8u, k8 = (unsigned)k*8u;

    int bmarkers = 0, bkind1 = 0;
    // LDS addresses of the traces of every facet (swe_flow_rhs_facets): component 0's pair, the others follow from it - 3*256 apart in
    // the planes, 1 apart in the staging area (six registers less than one pair per component: what three workgroups per CU need)
    unsigned tr[3][1];
    double h[3], nx[3], ny[3], u[3], v[3], e[3];
    if (real) {
        int nb[3], vid[3];
        swe_conn_load(p.idxc, p.idx4, p.idx2, k, nb, vid);
        bmarkers = (nb[0] < 0 ? -nb[0] : 0) | (nb[1] < 0 ? (-nb[1]) << 8 : 0) | (nb[2] < 0 ? (-nb[2]) << 16 : 0);
        if (bmarkers != 0) {
            const int m1 = (bmarkers & 0xff) ? (bmarkers & 0xff) : ((bmarkers & 0xff00) ? ((bmarkers >> 8) & 0xff) : (bmarkers >> 16));
            bkind1 = m1 < SWE_MAX_MARKERS ? p.bc.kind[m1] : 0;
        }
        const swe_rsrc_t gu = swe_rsrc(p.uin), gv = swe_rsrc(p.uin + 3*S), ge = swe_rsrc(p.uin + 6*S);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            u[i] = swe_ld(gu, k8, i*S8);
            v[i] = swe_ld(gv, k8, i*S8);
            e[i] = swe_ld(ge, k8, i*S8);
        }
        double r0[3][6];
        bool outside[3];
#pragma unroll
        for (int f = 0; f < 3; f++) {
            const int nbf = nb[f];
            const unsigned w = ((unsigned)tl.y >> (SWE_FUSE_FBITS*f)) & 0x3ffu;
            outside[f] = (w & 0x200u) != 0u;
            const unsigned at = w & 0x1ffu;                                   // lane in the tile, or staging slot
            // the neighbour traverses the shared facet backwards: its node f2 sits on my node f + 1, its node (f2 + 1) % 3 on my node f
            const int f2 = nbf >= 0 ? (nbf & 3) : f, f2a = f2 == 2 ? 0 : f2 + 1;
            {
                const unsigned ab = outside[f] ? (unsigned)(SWE_FUSE_XG + 6*at) : (unsigned)(f2*SWE_FUSE_WG + at);
                const unsigned aa = outside[f] ? (unsigned)(SWE_FUSE_XG + 6*at + 3) : (unsigned)(f2a*SWE_FUSE_WG + at);
                tr[f][0] = ab | (aa << 16);
            }
            // (issued for every facet: a facet inside the tile reads this cell itself, value unused - no branch around the loads)
            const int code = outside[f] ? nbf : ((k << 2) | f);
            const unsigned kn8 = (unsigned)(code >> 2)*8u;
            const int g2 = code & 3;
            const unsigned ob = kn8 + (g2 == 0 ? 0u : (g2 == 1 ? S8 : 2u*S8));         // node g2
            const unsigned oa = kn8 + (g2 == 0 ? S8 : (g2 == 1 ? 2u*S8 : 0u));         // node (g2 + 1) % 3
            r0[f][0] = swe_ld(gu, ob, 0); r0[f][1] = swe_ld(gv, ob, 0); r0[f][2] = swe_ld(ge, ob, 0);
            r0[f][3] = swe_ld(gu, oa, 0); r0[f][4] = swe_ld(gv, oa, 0); r0[f][5] = swe_ld(ge, oa, 0);
        }
        double px[3], py[3];
        const swe_rsrc_t rvx = swe_rsrc(p.vx), rvy = swe_rsrc(p.vy), rvh = swe_rsrc(p.vh);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const unsigned v8 = (unsigned)vid[i]*8u;
            px[i] = swe_ld(rvx, v8, 0);
            py[i] = swe_ld(rvy, v8, 0);
            h[i] = swe_ld(rvh, v8, 0);
        }
#pragma unroll
        for (int f = 0; f < 3; f++) {
            const int b = (f + 1) % 3;
            nx[f] = py[b] - py[f];
            ny[f] = px[f] - px[b];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) { lds[i*SWE_FUSE_WG + lane] = u[i]; lds[(3 + i)*SWE_FUSE_WG + lane] = v[i]; lds[(6 + i)*SWE_FUSE_WG + lane] = e[i]; }
#pragma unroll
        for (int f = 0; f < 3; f++) {
            if (outside[f]) {
                const unsigned at = ((unsigned)tl.y >> (SWE_FUSE_FBITS*f)) & 0x1ffu;
#pragma unroll
                for (int j = 0; j < 6; j++) lds[SWE_LDSI(SWE_FUSE_XG + 6*at + j, SWE_FUSE_LDS)] = r0[f][j];
            }
        }
    }
    __syncthreads();
    // ---- stage 1 on every cell of the tile: U(1) = U(0) + beta1 dt M^-1 R(U(0))
    double o1u[3], o1v[3], o1e[3];
    double twoA = 0.0;
    if (real) {
        twoA = fma(nx[0], ny[1], -(ny[0]*nx[1]));
        double bu[3], bv[3], be[3], wu[3], wv[3], we[3];
        double H[3];
        swe_tri_depths<NONLIN, false>(h, e, nullptr, H);
        swe_tri_cell<NONLIN>(p.g, u, v, e, H, nx, ny, bu, bv, be);
        swe_flow_rhs_facets<NONLIN, LF, SRC, 1, false, SWE_FUSE_XG, SWE_FUSE_WG, SWE_FUSE_LDS>(p, k, u, v, e, h, lds, tr, bmarkers, nx, ny, twoA, bu, bv, be);
#pragma unroll
        for (int i = 0; i < 3; i++) { wu[i] = 1.0*u[i]; wv[i] = 1.0*v[i]; we[i] = 1.0*e[i]; }
        swe_tri_finish<NONLIN, LF, false, true>(p, k, q.beta1, twoA, u, v, e, h, nullptr, nullptr, nx, ny, bmarkers, bkind1, bu, bv, be,
                                                wu, wv, we, true, o1u, o1v, o1e);
    }
    __syncthreads();                                       // every lane has read its traces of U(0)
    if (real) {
#pragma unroll
        for (int i = 0; i < 3; i++) { lds[i*SWE_FUSE_WG + lane] = o1u[i]; lds[(3 + i)*SWE_FUSE_WG + lane] = o1v[i]; lds[(6 + i)*SWE_FUSE_WG + lane] = o1e[i]; }
    }
    const bool act2 = lane < n_inner && k < q.cell_end;    // (a partition: stage 2's range ends before stage 1's)
    if (act2) {                                            // the part of stage 2's combine that does not depend on its tendency; U(0) is dead after this
#pragma unroll
        for (int i = 0; i < 3; i++) {
            lw[i][lane] = fma(q.a0_2, u[i], q.a1_2*o1u[i]);
            lw[3 + i][lane] = fma(q.a0_2, v[i], q.a1_2*o1v[i]);
            lw[6 + i][lane] = fma(q.a0_2, e[i], q.a1_2*o1e[i]);
        }
    }
    __syncthreads();
    // ---- stage 2 on the interior cells (every neighbour is a cell of the tile): U(2) = a0 U(0) + a1 U(1) + beta2 dt M^-1 R(U(1))
    if (act2) {
        // opaque to the optimiser (as in swe_flow_kernel): what stage 1 derived from the geometry - facet lengths, reciprocals,
        // gradients - would otherwise stay live across the barrier for stage 2, past the register budget of three waves per SIMD
#pragma unroll
        for (int i = 0; i < 3; i++) asm volatile("" : "+v"(nx[i]), "+v"(ny[i]), "+v"(h[i]));
#pragma unroll
        for (int f = 0; f < 3; f++) asm volatile("" : "+v"(tr[f][0]));
        asm volatile("" : "+v"(bmarkers), "+v"(twoA));
        double bu[3], bv[3], be[3], wu[3], wv[3], we[3], ou[3], ov[3], oe[3];
        double H[3];
        swe_tri_depths<NONLIN, false>(h, o1e, nullptr, H);
        swe_tri_cell<NONLIN>(p.g, o1u, o1v, o1e, H, nx, ny, bu, bv, be);
        swe_flow_rhs_facets<NONLIN, LF, SRC, 1, false, SWE_FUSE_XG, SWE_FUSE_WG, SWE_FUSE_LDS>(p, k, o1u, o1v, o1e, h, lds, tr, bmarkers, nx, ny, twoA, bu, bv, be);
#pragma unroll
        for (int i = 0; i < 3; i++) { wu[i] = lw[i][lane]; wv[i] = lw[3 + i][lane]; we[i] = lw[6 + i][lane]; }
        swe_tri_finish<NONLIN, LF, false, true>(p, k, q.beta2, twoA, o1u, o1v, o1e, h, nullptr, nullptr, nx, ny, bmarkers, bkind1, bu, bv, be,
                                                wu, wv, we, true, ou, ov, oe);
        const swe_rsrc_t gou = swe_rsrc(q.out), gov = swe_rsrc(q.out + 3*S), goe = swe_rsrc(q.out + 6*S);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            swe_st(gou, k8, i*S8, ou[i]);
            swe_st(gov, k8, i*S8, ov[i]);
            swe_st(goe, k8, i*S8, oe[i]);
        }
    }
}

// ---- all THREE stages of a step in one launch: two rings per tile (round 6, VERDICT r05 "next 2d") ---------------------------------
// A tile = interior cells (lanes 0 .. n_inner-1) + ring 1 (their facet neighbours, lanes n_inner .. n_mid-1) + ring 2 (the facet
// neighbours of ring 1, lanes n_mid .. n_all-1), 256 lanes in all.  Stage 1 on every cell of the tile (ring 2's outer neighbours'
// traces gathered from the state planes), stage 2 on interior + ring 1, stage 3 on the interior: U(1) and U(2) never leave the chip,
// per interior cell the launch reads U(0) once (x the tile's redundancy) and writes U(3).  U(3) goes to ANOTHER buffer than U(0) -
// a tile reads ring cells whose owners may already have finished - and the host swaps the two pointers after the launch.
// LDS: P0 [9][256] = U(0) (traces of stage 1; every lane's own U(0) for the Shu-Osher weights of stages 2 and 3), P1 [9][256] = the
// running stage values (U(1), then U(2)), then the staging area of the traces from outside the tile: 36.9 KB + 6 x 8 B per slot.
// The arithmetic of a cell is swe2d_tri.h's: the bits of the stage launches (tests/test_gpu_parity.py::test_fused_stage_triple...).
//
// Roles and lanes (round 10).  The ROLES of a tile are numbered [interior | ring 1 | ring 2 | padding]; role r sits on the physical
// lane (r + 64*rot) & 255, rot in 0..3 per tile, kept in counts[tile].y >> 16 (swe2d_tiles.h: SWE_FUSE3_ROT).  Stage 2 runs the roles
// below n_mid (~214 on the bench mesh), stage 3 those below n_inner (~176): the wave that holds the last 64 roles executes two stage
// bodies where the others execute three, and with rot = 0 everywhere that is wave 3 of every workgroup.  Everything the table says
// about lanes - the neighbour-lane fields, hence the LDS planes - is physical; only the two activity tests look at the role.
//
// The cell constants (round 10).  What a stage body derives from the mesh alone - the three facet lengths, their reciprocals and
// 1/twoA, 44 of its ~511 FP64 instructions - stage 1 leaves in LDS as it forms them (SWE_GEOM_KEEP of swe2d_flow.h), plane by plane
// ([7][256] by physical lane behind P1: conflict-free), and stages 2 and 3 read them where they are used (SWE_GEOM_STORED) instead of
// evaluating them again: no register lives longer for it.  The room is the staging area's, which moves INTO P1: nobody reads or writes
// P1 before stage 1's results go there, and those now wait for one more barrier (every lane has read its traces of U(0)).
// 25 planes of 256 doubles = 51.2 KB, three workgroups per CU as before (47.6 KB).
//
// The staging area (round 22) has the layout of the state planes (swe2d_tiles.h: kStagingPlanes): the lane that gathers a slot writes
// the slot's six values at its OWN index of six planes of P1 - component c on the reader's node f + 1 to plane 3c, on its node f to
// plane 3c + 1 - as it writes its own state to P0: conflict-free, and no slot number is formed.  Every trace of stage 1 is then 3*256
// doubles from the previous component's, outside the tile as inside: stage 1 takes SWE_TR_BYTES_INSIDE as stages 2 and 3 do, the
// select of the component step and its additions (24 integer VALU per body) go, and the DS offsets are immediates.  Which slot a lane
// gathers, if any, it reads from a third plane of its record (lane_slot), next to the other two: nothing waits for a per-tile word first.
#ifndef SWE_FUSE3_MAX_OUT
#define SWE_FUSE3_MAX_OUT 224                           // staging slots (a ring-2 cell has at most two facets towards the outside)
#endif
#ifndef SWE_FUSE3_GEOM
#define SWE_FUSE3_GEOM 1                                // 0: the layout and the arithmetic of round 6 - staging area behind P1, no records (A/B builds)
#endif
#define SWE_FUSE3_NGEO 7                                // Lf[3], 1/Lf[3], 1/twoA
#define SWE_FUSE3_GEO (18*SWE_FUSE_WG)                  // the records follow P0 and P1
#ifndef SWE_FUSE3_STAGING_PLANES
#define SWE_FUSE3_STAGING_PLANES 1                      // 0: the staging area of rounds 6-21, [slot][6] (A/B builds)
#endif
#define SWE_FUSE3_XG (SWE_FUSE3_GEOM ? 9*SWE_FUSE_WG : 18*SWE_FUSE_WG)       // the staging area: P1 while stage 1 runs
#define SWE_FUSE3_XG_DOUBLES (SWE_FUSE3_STAGING_PLANES ? 8*SWE_FUSE_WG : 6*SWE_FUSE3_MAX_OUT)
#define SWE_FUSE3_LDS (SWE_FUSE3_GEOM ? SWE_FUSE3_GEO + SWE_FUSE3_NGEO*SWE_FUSE_WG : SWE_FUSE3_XG + SWE_FUSE3_XG_DOUBLES)
static_assert(SWE_FUSE3_XG_DOUBLES <= 9*SWE_FUSE_WG, "the staging area must fit P1");
static_assert(SWE_FUSE3_MAX_OUT <= 4*(SWE_FUSE_WG/4 - 1) + 4 && SWE_FUSE3_MAX_OUT <= SWE_FUSE_WG, "a lane per staging slot");
#ifndef SWE_FUSE3_SRC_MIN_WG
#define SWE_FUSE3_SRC_MIN_WG 2                          // the source-term instances need 187-199 VGPRs: two workgroups per CU (at three: 80-132 B of scratch per lane)
#endif

struct SweFuse3Args {
    SweStageArgs st;          // uin = U(0) (state buffer A); geometry, connectivity, boundary tables; dt, g, sigma_lf
    const int4 *rec;          // [n_tiles][2][256]: the lane records, decoded on the host (swe2d_tiles.h: build_lane_records) - {cell or -1, the
                              //  three tr words of swe_flow_rhs_facets in bytes}, {8*vertex id x 3, bmarkers}
    const int2 *counts;       // [n_tiles]: {n_inner, n_mid | rot << 16}: roles 0 .. n_inner-1 interior, .. n_mid-1 ring 1; role r on lane (r + 64 rot) & 255
    const uint2 *lane_slot;   // [n_tiles][256]: by physical lane, the byte offsets into the state planes of the two nodes on the shared facet
                              //  of the staging slot this lane gathers, or {~0u, ~0u}: no slot (swe2d_tiles.h: LaneRecords::lane_slot)
    int n_tiles;
    int cell_end;             // stage 3 (the only one that leaves the chip) on cells [0, cell_end): a partition's last stage range
    double a0[3], a1[3], beta[3];   // Shu-Osher weights per stage (swe2d_ssprk33_coefficients)
    double *out;              // 9 planes: U(3), NOT the buffer of U(0)
};

#ifdef SWE_WAVE_TIMING
// profiling build only (tools/fuse3_phases.py): the phases of a tile's life.  Every wave of a sample of workgroups spread evenly over the
// launch stamps the shader clock (s_memtime) at SWE_F3P_STAMPS points, keeps the stamps in scalar registers and writes them behind its
// last store: swe_fuse3_phase[sample][wave] = {13 stamps, tile, HW_ID | XCC_ID << 32 | flags, 0}.  A stamp waits for its own return
// (lgkmcnt(0), which also drains the wave's LDS operations) and, where it marks an arrival, takes the arrived registers as operands, so
// that the compiler's own wait for exactly those loads stands in front of it.  The stamps cost time (about a tenth by the clock's
// documentation) and forbid overlaps the production kernel has: read shares, not lengths.
//    0 entry | 1 lane record arrived | 2 the cell's own state and vertices arrived | 3 the slot's six outside traces arrived (a wave
//    with a slot lane) | 4 behind barrier 1 | 5 end of stage 1's body | 6 behind barrier 2 | 7 behind barrier 3 (P1 written) |
//    8 end of stage 2's body | 9 behind barrier 4 | 10 behind barrier 5 (P1 written) | 11 end of stage 3's body | 12 stores drained
#define SWE_F3P_STAMPS 13
#define SWE_F3P_WORDS 16
#define SWE_F3P_MAX_WG 8192
__device__ unsigned long long swe_fuse3_phase[SWE_F3P_MAX_WG][4][SWE_F3P_WORDS];
#define SWE_F3T(i, ...) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wt[i]) : __VA_ARGS__ : "memory")
#define SWE_F3T9(i, a, b, c) SWE_F3T(i, "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(c[0]), "v"(c[1]), "v"(c[2]))
#else
#define SWE_F3T(i, ...)
#define SWE_F3T9(i, a, b, c)
#endif

template <bool NONLIN, bool LF, bool SRC = false>
__global__ __launch_bounds__(SWE_FUSE_WG, SRC ? SWE_FUSE3_SRC_MIN_WG : SWE_FUSE_MIN_WG) void swe_fuse123_kernel(const SweFuse3Args q)
{
#pragma clang fp contract(off)
    __shared__ double lds[SWE_FUSE3_LDS];
#ifdef SWE_WAVE_TIMING
    unsigned long long wt[SWE_F3P_STAMPS] = {};
    SWE_F3T(0, "s"(0));
#endif
    const SweStageArgs &p = q.st;
    const int tile = swe_logical_block(blockIdx.x, gridDim.x);
    if (tile >= q.n_tiles) return;                         // padding of the grid to a multiple of 8
    const int lane = (int)threadIdx.x;
    // the lane's record (swe2d_tiles.h: build_lane_records): decoded on the host, once per table - nothing here unpacks connectivity,
    // forms an LDS address or looks at a neighbour code (round 20)
    const int4 *const rec = q.rec + (size_t)tile*(2*SWE_FUSE_WG) + lane;
    const int4 ra = rec[0];                                // {cell or -1, tr[0..2]}
    const int4 rb = rec[SWE_FUSE_WG];                      // {8*vertex 0..2, bmarkers}
    const bool real = ra.x >= 0;
    const int k = real ? ra.x : 0;
    const int2 cnt = q.counts[tile];
    const int n_inner = cnt.x, n_mid = cnt.y & 0xffff, rot64 = (cnt.y >> 16) << 6;
    const size_t S = p.stride;
    const unsigned S8 = (unsigned)S*8u, k8 = (unsigned)k*8u;
    double *const P1 = lds + 9*SWE_FUSE_WG;
#ifdef SWE_WAVE_TIMING
    int wt_bodies = __any(real) ? 1 : 0;                   // profiling build only (tools/fuse3timing.py): stage bodies this wave executes
#endif
    // The traces from outside the tile are gathered by SLOT, not by lane and facet (round 19): only ring 2 has facets towards the outside,
    // ~84 slots of a bench tile, where a gather per lane and facet issued 18 loads in every lane for the ~500 of 4608 that were read.
    // Slot s is the work of physical lane 64*(s & 3) + (s >> 2): the slots are dealt round over the four waves, whatever the tile's
    // rotation - each wave, hence each SIMD, issues the six loads once with a quarter of the slots' lanes active, and the barrier behind
    // the prologue waits for four equal shares instead of one or two full waves (224 slots at most: 56 lanes of a wave).
    // Which slot that is the lane does not ask: its two byte offsets into the state planes lie in the third plane of its record, loaded
    // with the other two (round 22) - the six loads below are the second trip to memory, as the cell's own are, not the third.
    const uint2 so = q.lane_slot[(size_t)tile*SWE_FUSE_WG + lane];
    const bool has_slot = so.x != 0xffffffffu;
    SWE_F3T(1, "v"(ra.x), "v"(rb.x), "v"(so.x));

    int bmarkers = rb.w, bkind1 = 0;
    // per facet the BYTE addresses of component 0's two traces (swe_flow_rhs_facets, SWE_TR_BYTES): 16 bits each
    unsigned tr[3][1] = {{(unsigned)ra.y}, {(unsigned)ra.z}, {(unsigned)ra.w}};
    double h[3], nx[3], ny[3], u[3], v[3], e[3];
    double px[3], py[3];
    const swe_rsrc_t gu = swe_rsrc(p.uin), gv = swe_rsrc(p.uin + 3*S), ge = swe_rsrc(p.uin + 6*S);
    if (real) {
        if (bmarkers != 0) {                               // (a look-up, not a record field: swe2d_set_bc changes a marker's kind under a built table)
            const int m1 = (bmarkers & 0xff) ? (bmarkers & 0xff) : ((bmarkers & 0xff00) ? ((bmarkers >> 8) & 0xff) : (bmarkers >> 16));
            bkind1 = m1 < SWE_MAX_MARKERS ? p.bc.kind[m1] : 0;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            u[i] = swe_ld(gu, k8, i*S8);
            v[i] = swe_ld(gv, k8, i*S8);
            e[i] = swe_ld(ge, k8, i*S8);
        }
        const swe_rsrc_t rvx = swe_rsrc(p.vx), rvy = swe_rsrc(p.vy), rvh = swe_rsrc(p.vh);
        const unsigned v8[3] = {(unsigned)rb.x, (unsigned)rb.y, (unsigned)rb.z};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            px[i] = swe_ld(rvx, v8[i], 0);
            py[i] = swe_ld(rvy, v8[i], 0);
            h[i] = swe_ld(rvh, v8[i], 0);
        }
    }
    double r0[6];
    if (has_slot) {                                        // issued behind the cell's own loads, before anything waits for those
        const unsigned ob = so.x, oa = so.y;               // the source's node on the reader's node f + 1 / on its node f
        r0[0] = swe_ld(gu, ob, 0); r0[1] = swe_ld(gv, ob, 0); r0[2] = swe_ld(ge, ob, 0);
        r0[3] = swe_ld(gu, oa, 0); r0[4] = swe_ld(gv, oa, 0); r0[5] = swe_ld(ge, oa, 0);
    }
    if (real) {
#ifdef SWE_WAVE_TIMING
        SWE_F3T9(2, px, py, h);                            // (the last loads issued for the cell itself; loads return in order)
        SWE_F3T9(2, u, v, e);
#endif
#pragma unroll
        for (int f = 0; f < 3; f++) {
            const int b = (f + 1) % 3;
            nx[f] = py[b] - py[f];
            ny[f] = px[f] - px[b];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) { lds[i*SWE_FUSE_WG + lane] = u[i]; lds[(3 + i)*SWE_FUSE_WG + lane] = v[i]; lds[(6 + i)*SWE_FUSE_WG + lane] = e[i]; }
    }
    if (has_slot) {
        SWE_F3T(3, "v"(r0[0]), "v"(r0[1]), "v"(r0[2]), "v"(r0[3]), "v"(r0[4]), "v"(r0[5]));
#if SWE_FUSE3_STAGING_PLANES
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lds[SWE_LDSI(SWE_FUSE3_XG + 3*c*SWE_FUSE_WG + lane, SWE_FUSE3_LDS)] = r0[c];
            lds[SWE_LDSI(SWE_FUSE3_XG + (3*c + 1)*SWE_FUSE_WG + lane, SWE_FUSE3_LDS)] = r0[3 + c];
        }
#else
        const int slot = ((lane & 63) << 2) | (lane >> 6);
#pragma unroll
        for (int j = 0; j < 6; j++) lds[SWE_LDSI(SWE_FUSE3_XG + 6*slot + j, SWE_FUSE3_LDS)] = r0[j];
#endif
    }
    __syncthreads();
    SWE_F3T(4, "s"(0));
    // ---- stage 1 on every cell of the tile: U(1) = U(0) + beta1 dt M^-1 R(U(0)), into P1
    constexpr int GEOM1 = SWE_FUSE3_GEOM ? SWE_GEOM_KEEP : SWE_GEOM_COMPUTE, GEOM23 = SWE_FUSE3_GEOM ? SWE_GEOM_STORED : SWE_GEOM_COMPUTE;
    constexpr int TRB1 = SWE_FUSE3_STAGING_PLANES ? SWE_TR_BYTES_INSIDE : SWE_TR_BYTES;
    double twoA = 0.0;
    double *const G = lds + SWE_FUSE3_GEO + lane;          // the lane's record of cell constants: G[j*256]
    if (real) {
        twoA = fma(nx[0], ny[1], -(ny[0]*nx[1]));
        double bu[3], bv[3], be[3], wu[3], wv[3], we[3], ou[3], ov[3], oe[3];
        double H[3];
        swe_tri_depths<NONLIN, false>(h, e, nullptr, H);
        swe_tri_cell<NONLIN>(p.g, u, v, e, H, nx, ny, bu, bv, be);
        swe_flow_rhs_facets<NONLIN, LF, SRC, 1, false, SWE_FUSE3_XG, SWE_FUSE_WG, SWE_FUSE3_LDS, GEOM1, TRB1, true>(p, k, u, v, e, h, lds, tr, bmarkers, nx, ny, twoA, bu, bv, be,
                                                                                                     nullptr, nullptr, G);
#pragma unroll
        for (int i = 0; i < 3; i++) { wu[i] = 1.0*u[i]; wv[i] = 1.0*v[i]; we[i] = 1.0*e[i]; }
        swe_tri_finish<NONLIN, LF, false, true, GEOM1, SWE_FUSE_WG>(p, k, q.beta[0], twoA, u, v, e, h, nullptr, nullptr, nx, ny, bmarkers, bkind1,
                                                                    bu, bv, be, wu, wv, we, true, ou, ov, oe, G);
#pragma unroll
        for (int i = 0; i < 3; i++) { u[i] = ou[i]; v[i] = ov[i]; e[i] = oe[i]; }
        SWE_F3T9(5, u, v, e);
    }
    if (SWE_FUSE3_GEOM) __syncthreads();                   // every lane has read its traces of U(0): the staging area is P1 again
    SWE_F3T(6, "s"(0));
    if (real) {
#pragma unroll
        for (int i = 0; i < 3; i++) { P1[i*SWE_FUSE_WG + lane] = u[i]; P1[(3 + i)*SWE_FUSE_WG + lane] = v[i]; P1[(6 + i)*SWE_FUSE_WG + lane] = e[i]; }
    }
    __syncthreads();
    SWE_F3T(7, "s"(0));
    // ---- stage 2 on interior + ring 1, stage 3 on the interior: every neighbour is a cell of the tile, traces from P1; the lane's own
    //      U(0) for the weights from P0
    // One body, called once per stage with s a constant (round 22; a rolled loop before): the s == 1 arm, the compares that chose the
    // stage's bound and the copies u = ou that the loop carried round its back edge (9-10 v_mov_b64 per body) are gone.  168 VGPRs, no scratch.
    auto later_stage = [&](const int s) __attribute__((always_inline)) {
        const int role = (lane - rot64) & (SWE_FUSE_WG - 1);
        const bool act = role < (s == 1 ? n_mid : n_inner) && (s == 1 || k < q.cell_end);
#ifdef SWE_WAVE_TIMING
        wt_bodies += __any(act) ? 1 : 0;
#endif
        double ou[3], ov[3], oe[3];
        if (act) {
            // opaque to the optimiser (as in swe_flow_kernel): what the previous stage derived from the geometry would otherwise stay
            // live across the barrier, past the register budget of three waves per SIMD
#pragma unroll
            for (int i = 0; i < 3; i++) asm volatile("" : "+v"(nx[i]), "+v"(ny[i]), "+v"(h[i]));
#pragma unroll
            for (int f = 0; f < 3; f++) asm volatile("" : "+v"(tr[f][0]));
            asm volatile("" : "+v"(bmarkers));
            if (SRC || !SWE_FUSE3_GEOM) asm volatile("" : "+v"(twoA));     // (else nothing reads it after stage 1)
            double bu[3], bv[3], be[3], wu[3], wv[3], we[3];
            double H[3];
            swe_tri_depths<NONLIN, false>(h, e, nullptr, H);
            swe_tri_cell<NONLIN>(p.g, u, v, e, H, nx, ny, bu, bv, be);
            swe_flow_rhs_facets<NONLIN, LF, SRC, 1, false, SWE_FUSE3_XG, SWE_FUSE_WG, 9*SWE_FUSE_WG, GEOM23, SWE_TR_BYTES_INSIDE, true>(p, k, u, v, e, h, P1, tr, bmarkers, nx, ny, twoA, bu, bv, be,
                                                                                                          nullptr, nullptr, G);
            const double a0 = q.a0[s], a1 = q.a1[s];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                wu[i] = fma(a0, lds[i*SWE_FUSE_WG + lane], a1*u[i]);
                wv[i] = fma(a0, lds[(3 + i)*SWE_FUSE_WG + lane], a1*v[i]);
                we[i] = fma(a0, lds[(6 + i)*SWE_FUSE_WG + lane], a1*e[i]);
            }
            swe_tri_finish<NONLIN, LF, false, true, GEOM23, SWE_FUSE_WG>(p, k, q.beta[s], twoA, u, v, e, h, nullptr, nullptr, nx, ny, bmarkers,
                                                                         bkind1, bu, bv, be, wu, wv, we, true, ou, ov, oe, G);
#ifdef SWE_WAVE_TIMING
            if (s == 1) SWE_F3T9(8, ou, ov, oe); else SWE_F3T9(11, ou, ov, oe);
#endif
        }
        if (s == 1) {
            __syncthreads();                               // every lane has read its traces of U(1)
            SWE_F3T(9, "s"(0));
            if (act) {
#pragma unroll
                for (int i = 0; i < 3; i++) { P1[i*SWE_FUSE_WG + lane] = ou[i]; P1[(3 + i)*SWE_FUSE_WG + lane] = ov[i]; P1[(6 + i)*SWE_FUSE_WG + lane] = oe[i]; }
#pragma unroll
                for (int i = 0; i < 3; i++) { u[i] = ou[i]; v[i] = ov[i]; e[i] = oe[i]; }
            }
            __syncthreads();
            SWE_F3T(10, "s"(0));
        } else if (act) {
            const swe_rsrc_t gou = swe_rsrc(q.out), gov = swe_rsrc(q.out + 3*S), goe = swe_rsrc(q.out + 6*S);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                swe_st(gou, k8, i*S8, ou[i]);
                swe_st(gov, k8, i*S8, ov[i]);
                swe_st(goe, k8, i*S8, oe[i]);
            }
        }
    };
    later_stage(1);
    later_stage(2);
#ifdef SWE_WAVE_TIMING
    // where did the wave run, and how much of the tile's work did it do?  HW_ID | XCC_ID << 32 | stage bodies << 40 | 1 << 44, per
    // wave of the launch: swe_wave_ts read as one array of 6*SWE_WT_MAX words, word 4*blockIdx.x + wave
    if ((lane & 63) == 0 && 4*blockIdx.x + (lane >> 6) < 6*SWE_WT_MAX) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        (&swe_wave_ts[0][0])[4*blockIdx.x + (lane >> 6)] = (unsigned long long)hw | ((unsigned long long)(xcc & 0xf) << 32)
                                                           | ((unsigned long long)wt_bodies << 40) | (1ull << 44);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the stores of stage 3 have left
    SWE_F3T(12, "s"(0));
    const unsigned wt_every = (gridDim.x + SWE_F3P_MAX_WG - 1)/SWE_F3P_MAX_WG;
    if ((lane & 63) == 0 && blockIdx.x % wt_every == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long *const w = swe_fuse3_phase[blockIdx.x/wt_every][lane >> 6];
#pragma unroll
        for (int i = 0; i < SWE_F3P_STAMPS; i++) w[i] = wt[i];
        w[13] = (unsigned long long)tile;
        w[14] = (unsigned long long)hw | ((unsigned long long)(xcc & 0xf) << 32) | ((unsigned long long)wt_bodies << 40) | (1ull << 44);
        w[15] = 0ull;
    }
#endif
}

// (Round 6, measured and removed: the three stages of a TRACER step in one launch on these two-ring tiles - the tracer in LDS between
//  the stages, the velocity traces in registers, bit for bit the stage launches.  Slower at every size: tracer only at 1 M cells 89.7
//  against 78.0 us per step, at 4 M 424.9 against 391.6 - profiles/r06d_cfgs*.txt, r06e_cfgs_4m.txt, DESIGN_ANNEX.md A8.)
//
// (Round 6, measured and not kept: tile records that carried the cell's PACKED connectivity - 32 B per lane, two int4 - so that a lane
//  issued its loads after ONE trip to memory instead of two (tile entry, then the connectivity record).  That removed the trip and
//  nothing else: every lane still unpacked the record and formed its addresses from it, and the table grew by 12 B per cell.  2-6 %
//  slower at 250 k ... 4 M cells - profiles/r06f_fused_sizes.txt against r06b_fused_sizes.txt.  The lane records of round 20 above
//  have the same size and hold the DECODED words: the trip and the decode both go.)

// ---- stages 1 and 2 of a step in one launch on QUADRILATERALS (round 6): the triangle kernel's tiles with four facets per cell ------
// 256 lanes = up to 192 interior cells + their ring of at most 64 (a 16 x 12 tile of a structured mesh: ring 56); the arithmetic is
// swe_quad_stage_cell, the function the stage launches call - the same bits (tests/test_quads.py::test_fused_stage_pair_on_quad...).
// LDS: [12][256] stage values (u0..3 v0..3 e0..3 of every lane: U(0), then U(1)), the staging area of the traces from outside the tile
// ([slot][6]: u, v, e at the neighbour's node on my node f + 1, then at its node on my node f), and [12][192] = U(0) of the interior
// lanes for stage 2's Shu-Osher weights: 52.2 KB, three workgroups per CU.  At 1 M quadrilaterals the three state buffers (288 MB) do
// not fit the Infinity Cache: the two stage launches this replaces move 592 B per cell, the fused launch ~290.
#define SWE_QFUSE_INNER 192
#define SWE_QFUSE_RING (SWE_FUSE_WG - SWE_QFUSE_INNER)
#define SWE_QFUSE_XG (12*SWE_FUSE_WG)
#define SWE_QFUSE_MAX_OUT (3*SWE_QFUSE_RING)            // a ring cell has a facet towards the interior: at most three towards the outside
#define SWE_QFUSE_LDS (SWE_QFUSE_XG + 6*SWE_QFUSE_MAX_OUT)

struct SweFuseQuadArgs {
    SweStageArgs st;          // uin = U(0) (state buffer A); geometry, connectivity planes, boundary tables; dt, g, sigma_lf
    const int4 *tile;         // [n_tiles][256]: {cell or -1, facets 0-2 (10 bits each: lane of the neighbour in the tile - a boundary facet:
                              //  the lane itself - or bit 9 + staging slot), facet 3, 0}
    const int *n_inner;       // [n_tiles]
    int n_tiles;
    int cell_end;             // stage 2 updates the interior cells < cell_end
    double beta1, a0_2, a1_2, beta2;
    double *out;              // 12 planes: U(2) (state buffer C)
};

template <bool NONLIN, bool LF, bool SRC, bool AFFINE>
__global__ __launch_bounds__(SWE_FUSE_WG, SWE_FUSE_MIN_WG) void swe_fuse12_quad_kernel(const SweFuseQuadArgs q)
{
#pragma clang fp contract(off)
    __shared__ double lds[SWE_QFUSE_LDS];
    __shared__ double lu0[12*SWE_QFUSE_INNER];
    const SweStageArgs &p = q.st;
    const int tile = swe_logical_block(blockIdx.x, gridDim.x);
    if (tile >= q.n_tiles) return;
    const int lane = (int)threadIdx.x;
    const int4 tl = q.tile[(size_t)tile*SWE_FUSE_WG + lane];
    const bool real = tl.x >= 0;
    const int k = real ? tl.x : 0;
    const int n_inner = q.n_inner[tile];
    const size_t S = p.stride;
    const unsigned S8 = (unsigned)S*8u, k8 = (unsigned)k*8u, S4 = (unsigned)S*4u, k4 = (unsigned)k*4u;

    unsigned tr[4] = {0u, 0u, 0u, 0u}, bmarkers = 0u;
    int nb[4] = {-1, -1, -1, -1}, vid[4] = {0, 0, 0, 0};
    double u[4], v[4], e[4];
    if (real) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            nb[i] = swe_ldi(swe_rsrc(p.nbr), k4, i*S4);
            vid[i] = swe_ldi(swe_rsrc(p.cv), k4, i*S4);
        }
        const swe_rsrc_t gu = swe_rsrc(p.uin), gv = swe_rsrc(p.uin + 4*S), ge = swe_rsrc(p.uin + 8*S);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            u[i] = swe_ld(gu, k8, i*S8);
            v[i] = swe_ld(gv, k8, i*S8);
            e[i] = swe_ld(ge, k8, i*S8);
        }
        bmarkers = (nb[0] < 0 ? (unsigned)(-nb[0]) : 0u) | (nb[1] < 0 ? (unsigned)(-nb[1]) << 8 : 0u) |
                   (nb[2] < 0 ? (unsigned)(-nb[2]) << 16 : 0u) | (nb[3] < 0 ? (unsigned)(-nb[3]) << 24 : 0u);
        double r0[4][6];
        bool outside[4];
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const int nbf = nb[f];
            const unsigned w = f < 3 ? (((unsigned)tl.y >> (SWE_FUSE_FBITS*f)) & 0x3ffu) : ((unsigned)tl.z & 0x3ffu);
            outside[f] = (w & 0x200u) != 0u;
            const unsigned at = w & 0x1ffu;                                   // lane in the tile, or staging slot
            // the neighbour traverses the shared facet backwards: its node f2 sits on my node f + 1, its node (f2 + 1) & 3 on my node f
            const int f2 = nbf >= 0 ? (nbf & 3) : f, na = (f2 + 1) & 3;
            const unsigned ab = outside[f] ? (unsigned)(SWE_QFUSE_XG + 6*at) : (unsigned)(f2*SWE_FUSE_WG + at);
            const unsigned aa = outside[f] ? (unsigned)(SWE_QFUSE_XG + 6*at + 3) : (unsigned)(na*SWE_FUSE_WG + at);
            tr[f] = ab | (aa << 16);
            // (issued for every facet: a facet inside the tile reads this cell itself, value unused - no branch around the loads)
            const int code = outside[f] ? nbf : ((k << 2) | f);
            const unsigned kn8 = (unsigned)(code >> 2)*8u;
            const int g2 = code & 3, ga = (g2 + 1) & 3;
            const unsigned ob = kn8 + ((g2 & 1) ? S8 : 0u) + ((g2 & 2) ? 2u*S8 : 0u);
            const unsigned oa = kn8 + ((ga & 1) ? S8 : 0u) + ((ga & 2) ? 2u*S8 : 0u);
            r0[f][0] = swe_ld(gu, ob, 0); r0[f][1] = swe_ld(gv, ob, 0); r0[f][2] = swe_ld(ge, ob, 0);
            r0[f][3] = swe_ld(gu, oa, 0); r0[f][4] = swe_ld(gv, oa, 0); r0[f][5] = swe_ld(ge, oa, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { lds[i*SWE_FUSE_WG + lane] = u[i]; lds[(4 + i)*SWE_FUSE_WG + lane] = v[i]; lds[(8 + i)*SWE_FUSE_WG + lane] = e[i]; }
#pragma unroll
        for (int f = 0; f < 4; f++) {
            if (outside[f]) {
                const unsigned at = (f < 3 ? ((unsigned)tl.y >> (SWE_FUSE_FBITS*f)) : (unsigned)tl.z) & 0x1ffu;
#pragma unroll
                for (int j = 0; j < 6; j++) lds[SWE_LDSI(SWE_QFUSE_XG + 6*at + j, SWE_QFUSE_LDS)] = r0[f][j];
            }
        }
    }
    __syncthreads();
    // the six traces of facet f from LDS: component c is 4 planes further inside the tile, one double further in the staging area
#define SWE_QFUSE_TRACES(una, unb, vna, vnb, ena, enb) \
    _Pragma("unroll") \
    for (int f = 0; f < 4; f++) { \
        const unsigned ab = tr[f] & 0xffffu, aa = tr[f] >> 16; \
        const unsigned step = ab >= (unsigned)SWE_QFUSE_XG ? 1u : (unsigned)(4*SWE_FUSE_WG); \
        unb[f] = lds[SWE_LDSI(ab, SWE_QFUSE_LDS)]; vnb[f] = lds[SWE_LDSI(ab + step, SWE_QFUSE_LDS)]; enb[f] = lds[SWE_LDSI(ab + 2u*step, SWE_QFUSE_LDS)]; \
        una[f] = lds[SWE_LDSI(aa, SWE_QFUSE_LDS)]; vna[f] = lds[SWE_LDSI(aa + step, SWE_QFUSE_LDS)]; ena[f] = lds[SWE_LDSI(aa + 2u*step, SWE_QFUSE_LDS)]; \
    }
    // ---- stage 1 on every cell of the tile: U(1) = U(0) + beta1 dt M^-1 R(U(0))
    double o1u[4], o1v[4], o1e[4];
    if (real) {
        double una[4], unb[4], vna[4], vnb[4], ena[4], enb[4];
        SWE_QFUSE_TRACES(una, unb, vna, vnb, ena, enb)
        swe_quad_stage_cell<NONLIN, LF, false, SRC, false, AFFINE, true>(p, k, k8, S8, nb, vid, bmarkers, u, v, e, una, unb, vna, vnb, ena, enb,
                                                                        0.0, 1.0, q.beta1, lds, SWE_FUSE_WG, lane, nullptr, 0, o1u, o1v, o1e);
    }
    __syncthreads();                                       // every lane has read its traces (and its boundary facets' inputs) of U(0)
    const bool act2 = lane < n_inner && k < q.cell_end;
    if (real) {
#pragma unroll
        for (int i = 0; i < 4; i++) { lds[i*SWE_FUSE_WG + lane] = o1u[i]; lds[(4 + i)*SWE_FUSE_WG + lane] = o1v[i]; lds[(8 + i)*SWE_FUSE_WG + lane] = o1e[i]; }
    }
    if (act2) {
#pragma unroll
        for (int i = 0; i < 4; i++) { lu0[i*SWE_QFUSE_INNER + lane] = u[i]; lu0[(4 + i)*SWE_QFUSE_INNER + lane] = v[i]; lu0[(8 + i)*SWE_QFUSE_INNER + lane] = e[i]; }
    }
    __syncthreads();
    // ---- stage 2 on the interior cells (every neighbour is a cell of the tile): U(2) = a0 U(0) + a1 U(1) + beta2 dt M^-1 R(U(1))
    if (act2) {
#pragma unroll
        for (int f = 0; f < 4; f++) asm volatile("" : "+v"(tr[f]));
        asm volatile("" : "+v"(bmarkers));
        double una[4], unb[4], vna[4], vnb[4], ena[4], enb[4], ou[4], ov[4], oe[4];
        SWE_QFUSE_TRACES(una, unb, vna, vnb, ena, enb)
        swe_quad_stage_cell<NONLIN, LF, true, SRC, false, AFFINE, true>(p, k, k8, S8, nb, vid, bmarkers, o1u, o1v, o1e, una, unb, vna, vnb, ena, enb,
                                                                       q.a0_2, q.a1_2, q.beta2, lds, SWE_FUSE_WG, lane, lu0, SWE_QFUSE_INNER, ou, ov, oe);
        const swe_rsrc_t gou = swe_rsrc(q.out), gov = swe_rsrc(q.out + 4*S), goe = swe_rsrc(q.out + 8*S);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            swe_st(gou, k8, i*S8, ou[i]);
            swe_st(gov, k8, i*S8, ov[i]);
            swe_st(goe, k8, i*S8, oe[i]);
        }
    }
#undef SWE_QFUSE_TRACES
}
