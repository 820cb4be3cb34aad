// swe2d_plan.hip - how one SSPRK33 step is launched: which kernels cover a handle, which of them a caller takes, the tile tables that
// path needs.  Host code only.  Every path gives the same bits: the rule decides speed and which buffers hold U(1) / U(2) afterwards.
#include "swe2d_handle.h"

namespace swe2d_impl {

// ---- 1. coverage, from the handle's configuration alone (no HIP call, no allocation): what a kernel declines costs one line here
unsigned step_kernels(const Handle *h)
{
    const int mode = h->opt[SWE2D_OPT_FUSED_STAGES];
    unsigned k = kPair | kTriple | kFlow;
    // quadrilaterals: the stage pair alone (swe_fuse12_quad_kernel, round 6), on whole meshes
    if (h->npc != 3) k &= h->n_owned == h->n_cells ? kPair : 0u;
    if (h->npc == 3 && !h->idx4) k = 0;                      // triangles: every step kernel reads the packed connectivity
    // wetting-drying: the dataflow kernel since round 5 (swe_flow_kernel<..., WD>, nonlinear equations as in the stage kernels;
    // SWE2D_OPT_FLOW_WD = 0 leaves it to the stage launches), never the tiles
    if (h->wd) k &= (h->par.use_nonlinear_equations && opt_on(h, SWE2D_OPT_FLOW_WD)) ? kFlow : 0u;
    if (h->visc) k = 0;                                      // viscosity: a pass after each stage launch (swe2d_sipg.h)
    if (h->n_farms > 0) k = 0;                               // tidal turbine farms: the stage kernels carry the term (swe_source_terms<true>)
    if (h->tide.n > 0) k = 0;                                // tidal boundary table: one tide launch in front of every stage launch (step_swe)
    if (h->atm.n_t > 0) k = 0;                               // atmospheric record: the fields change per stage, a fused launch reads them once
    if (h->sed.on && h->sed.par.solve_exner) k &= ~kFlow;   // Exner: the bed moves after every step, the dataflow kernel batches steps
    if (h->bed.on) k &= ~kFlow;                              // bedload: a pass after every step, and with it the bed moves
    if (h->slide.on) k &= ~kFlow;                            // sediment slide: likewise
    if (h->opt[SWE2D_OPT_BND_INLINE] == 0) k = 0;            // the epilogue variant was asked for: stage kernels only
    if (h->h_nbr.empty()) k &= ~(kPair | kTriple);           // the tiles are cut from the host copy of the neighbour codes
    if (!h->flow_flag || !h->flow_ex) k &= ~kFlow;           // the dataflow kernel's tables (flow_build)
    // SWE2D_OPT_FUSED_STAGES: 0 never a tile kernel; 1, 2 never the three-stage one; 3 forces it.  By itself (-1) the three-stage
    // kernel stays away from source terms (those instances need 187-199 VGPRs: at three workgroups per CU they spill 80-132 B per
    // lane - 1 M cells 159-161 us per step by the pair, 235-239 by this kernel -, at two, as built, 195-196 against 163-164:
    // profiles/r06q_*)
    if (mode == 0) k &= ~(kPair | kTriple);
    if (mode != 3 && (mode != -1 || has_sources(h))) k &= ~kTriple;
    return k;
}

// ---- 2. the plan: sizes from which a kernel that covers the handle is taken by itself
// The dataflow kernel: up to 128 steps per launch without grid barriers (swe2d_flow.h) where every 64-cell block of the mesh is
// resident at once (131 072 cells = 2048 resident blocks; the test is flow_fits, by the device's own capacity) and the kernel covers
// the configuration.  Same box, us/step, three stage launches per step -> flow launches: 15 k cells 16.5 -> 15.3, 62 k 20.1 -> 15.1,
// 125 k 24.3 -> 18.3 (the one-launch step kernel of round 2, which this replaces: 14.1 / 16.8 / 24.9).  SWE2D_OPT_FLOW = 0 selects the
// stage launches (the same bits either way).
constexpr int kFlowMaxCells = 131072;
// The stage pair covers triangles without wetting-drying or viscosity - with or without source terms (the SRC instances keep the 168
// VGPRs / three workgroups per CU of the plain ones, tools/kres.py), the whole mesh or a partition's owned + ghost cells on its
// shrinking stage ranges (round 6); taken from
// 250 k cells, where a step streams from memory (same box, us per step, stage launches -> fused pair + stage 3, device numbering in
// 16 x 6-quad tiles: 125 k cells 23.9 -> 24.1, 250 k 38.8 -> 37.0, 500 k 64.9 -> 61.1, 1 M 121.0 -> 107.3, 2 M 264 -> 235, 4 M 525 -> 477;
// profiles/r05zl_fused_stage_pair.txt), and where the numbering gives tiles worth it (fuse12_tiles_pay).
// (In the range-checked build too since round 6: the shared functions test their LDS indices against the array they are handed, the
// tile tables are host-built indices.)
constexpr int kPairFromTriangles = 250000;
// quadrilaterals: from the size at which the three state buffers (3 x 96 B per cell) leave the Infinity Cache - same box, us per step
// without -> with: 1 M cells 188.9 -> 172.6, + Manning 221.1 -> 212.0, cfg 4 338.8 -> 329.3; 640 k cells 115.7 -> 114.6, + Manning
// 136.8 -> 142.7 (profiles/r06g_quads*.txt)
constexpr int kPairFromQuads = 850000;
// All three stages in one launch.  With tiles cut as consecutive cells of the numbering (147 + 52 + 57 per tile, ragged) the second ring
// costs 1.26 x the arithmetic of the pair and only pays where the state no longer fits the Infinity Cache - same box, us per step,
// three stage launches / fused pair + stage 3 / all three fused (profiles/r06b_fused_sizes.txt): 250 k cells 37.0 / 35.2 / 36.1,
// 1 M 110.0 / 103.0 / 110.8, 2 M 272.0 / 233.3 / 229.9, 4 M 527.9 / 475.3 / 452.1: by itself from 2.5 M cells.  With the caller's
// patches (swe2d_fused_set_triple_tiles: 11 x 8 quads of a RectangleMesh = 176 + 38 + 42 cells, every lane of the 256 used) it wins
// wherever the dataflow kernel does not apply (profiles/r06l_triple_tiles.txt, r06m_triple_sizes.txt): 150 k cells 28.3 / 27.5 / 24.1,
// 250 k 36.9 / 34.8 / 31.5, 500 k 62.4 / 57.9 / 53.8, 1 M - / 103.4 / 96.8, 2 M - / 235.4 / 207.5, 4 M - / 476.7 / 406.9: by itself
// beyond kFlowMaxCells.
constexpr int kTripleFromCells = 2500000;
constexpr int kForcedFromCells = 64;                       // SWE2D_OPT_FUSED_STAGES = 1 / 3: on every mesh of at least 64 cells, whatever its tiles
// tiles not worth it: the mean interior below 176 of 192 cells on a whole mesh (the structured tile order and the Hilbert order of an
// unstructured mesh pass - 1 M Delaunay triangles 192.0 + 49.9 cells per tile, 120.8 -> 113.3 us per step; an order that does not
// keeps its stage launches), below 150 on a partition (its tiles along the cuts and through the ghost layers are partial by construction)
constexpr double kPairMinInteriorWhole = 176.0, kPairMinInteriorPartition = 150.0;

static bool forced_pair(const Handle *h) { return h->opt[SWE2D_OPT_FUSED_STAGES] == 1 || h->opt[SWE2D_OPT_FUSED_STAGES] == 3; }
bool fuse12_tiles_pay(const Handle *h, int n_tiles)
{
    return forced_pair(h) || (double)h->n_cells/n_tiles >= (h->n_owned == h->n_cells ? kPairMinInteriorWhole : kPairMinInteriorPartition);
}
bool flow_fits(Handle *h) { return ((h->flow_blocks + 7)/8)*8 <= flow_capacity(h); }        // every block of a flow launch resident at once

StepPath step_plan(Handle *h, StepCaller who, StepPath at_most)
{
    const unsigned can = step_kernels(h);
    const int n = h->n_cells;
    const bool whole = who == kAdvance || who == kWholeStep;
    // only swe2d_advance takes the dataflow kernel
    if (who == kAdvance && at_most >= kFlow && (can & kFlow) && opt_on(h, SWE2D_OPT_FLOW) && flow_fits(h)) return kFlow;
    if (who != kPartitionPair && at_most >= kTriple && (can & kTriple) && (!whole || h->n_owned == n)) {
        const bool patches = (int)h->fuse3_start.size() == n;         // swe2d_fused_set_triple_tiles
        if (h->opt[SWE2D_OPT_FUSED_STAGES] == 3 ? (!whole || n >= kForcedFromCells)
                                                : ((patches && n > kFlowMaxCells) || (whole && n >= kTripleFromCells)))
            return kTriple;
    }
    if (who == kPartitionStep) return kStages;              // (the caller drives a partition's stage pair itself)
    if (at_most >= kPair && (can & kPair) && n >= (forced_pair(h) ? kForcedFromCells : (h->npc == 3 ? kPairFromTriangles : kPairFromQuads)))
        return kPair;
    return kStages;
}

// ---- 3. make it ready: the tile tables of the planned path.  Allocations and copies, so nothing is built inside a stream capture;
// a path without tables - first use inside a capture, tiles judged poor (fuse_state == -1) - gives way to the next one.
int step_ready(Handle *h, StepCaller who, StepPath at_most, StepPath *path)
{
    StepPath p = step_plan(h, who, at_most);
    if (p == kTriple) {
        if (int rc = fuse123_build(h)) return rc;
        if (!h->fuse3.tile) p = step_plan(h, who, kPair);
    }
    if (p == kPair) {
        if (int rc = fuse12_build(h)) return rc;
        if (!pair_tiles(h).tile) p = kStages;
    }
    *path = p;
    return SWE2D_OK;
}

int whole_step_path(Handle *h, StepCaller who, StepPath *path)
{
    // the three-stage launch swaps two state buffers on the host: not inside a stream capture, which keeps the pair or the stages
    const bool no_swap = step_plan(h, who) == kTriple && stream_capturing(h);
    return step_ready(h, who, no_swap ? kPair : kFlow, path);
}

int step_launch(Handle *h, StepPath path, int i)
{
    if (path == kTriple) return launch_fuse123(h, h->n_owned);
    if (path == kPair) return i == 0 ? launch_fuse12(h, h->n_owned) : stage_on_range(h, 2, 0, h->n_owned);
    return stage_on_range(h, i, 0, h->n_owned);
}

int forcing_refuse_capture(Handle *h)
{
    // the time is a kernel argument: a replay of the captured launches would repeat it
    if (forced(h) && stream_capturing(h))
        return fail(h, SWE2D_ERR_UNSUPPORTED, "a handle with a tide table or an atmospheric record cannot be stepped inside a stream capture (the time is a kernel argument)");
    return SWE2D_OK;
}

int step_swe(Handle *h, StepCaller who, int n_steps)
{
    StepPath path;
    if (n_steps <= 0) return SWE2D_OK;
    if (forced(h)) {
        // stage launches, the boundary elevation and the atmospheric fields of the stage's time in front of each; the clock moves on
        // by the steps made.  Nothing is enqueued unless every stage time lies inside the atmospheric record.
        if (int rc = forcing_refuse_capture(h)) return rc;
        if (int rc = atm_check_advance(h, n_steps, false)) return rc;
        for (int k = 0; k < n_steps; k++)
            for (int i = 0; i < 3; i++) {
                const double t = tide_stage_time(h, k, i);
                if (h->tide.n > 0) { if (int rc = tide_launch(h, t)) return rc; }
                if (h->atm.n_t > 0) { if (int rc = atm_launch(h, t)) return rc; }
                if (int rc = stage_on_range(h, i, 0, h->n_owned)) return rc;
            }
        h->clock_k_first += n_steps;
        return SWE2D_OK;
    }
    if (int rc = whole_step_path(h, who, &path)) return rc;
    if (path == kFlow) {
        int32_t ends[SWE_FLOW_MAX_STAGES];
        for (int s = 0; s < SWE_FLOW_MAX_STAGES; s++) ends[s] = h->n_owned;
        for (int done = 0; done < n_steps; done += SWE_FLOW_MAX_STAGES/3)
            if (int rc = launch_flow(h, 3*std::min(n_steps - done, SWE_FLOW_MAX_STAGES/3), ends)) return rc;
        return SWE2D_OK;
    }
    for (int l = 0; l < n_steps*launches_per_step(path); l++)
        if (int rc = step_launch(h, path, l % launches_per_step(path))) return rc;
    return SWE2D_OK;
}

}  // namespace swe2d_impl
