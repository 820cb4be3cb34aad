// swe2d_api_fuse.hip - stages 1 + 2 of a step in one launch by overlapped tiles (swe2d_fuse.h): instances, tile tables, launch
#include "swe2d_handle.h"
#include "swe2d_fuse.h"
#include "swe2d_tiles.h"

#include <type_traits>

namespace swe2d_impl {

namespace {
// run-time flags -> template arguments: pick_instance(f, a, b, c) = f(bool_constant<a>, bool_constant<b>, bool_constant<c>)
template <bool... B, class F> auto pick_instance(F f) { return f(std::bool_constant<B>{}...); }
template <bool... B, class F, class... Rest> auto pick_instance(F f, bool b, Rest... rest)
{
    return b ? pick_instance<B..., true>(f, rest...) : pick_instance<B..., false>(f, rest...);
}

// The tiles (swe2d_tiles.h) are cut from consecutive cells of the device numbering (compact patches in the tile-Hilbert order) - or of
// the order handed in with swe2d_fused_set_order: a partition's ghost layers are appended to its numbering layer by layer, strips one
// cell wide whose tiles would be all ring.  The stage pair: an interior of at most 192 cells, a ring of at most 64.  The three-stage
// kernel: interior + ring 1 + ring 2 fit the 256 lanes and ring 2's facets towards the outside the staging area - and a tile ends at the
// next position the caller marked as a start (swe2d_fused_set_triple_tiles: patches of 11 x 8 quads = 176 triangles + 38 + 42 fill the
// 256 lanes, where 147 consecutive cells of the 16 x 6 numbering leave ragged patches with rings of 52 + 57); role r of such a tile sits
// on the physical lane (r + 64*rot) & 255.
const TileSpec kPairTiles{3, 1, SWE_FUSE_WG, SWE_FUSE_INNER, SWE_FUSE_RING, SWE_FUSE_MAX_OUT, false};
const TileSpec kQuadPairTiles{4, 1, SWE_FUSE_WG, SWE_QFUSE_INNER, SWE_QFUSE_RING, SWE_QFUSE_MAX_OUT, false};
const TileSpec kTripleTiles{3, 2, SWE_FUSE_WG, SWE_FUSE_WG, -1, SWE_FUSE3_MAX_OUT, true, true};     // (rotated; wall cells on consecutive roles)

int build_table(Handle *h, const TileSpec &spec, const std::vector<int> &order, const std::vector<unsigned char> &start, TileTable &t)
{
    const int n = h->n_cells;
    std::string err;
    if (build_tiles(h->h_nbr.data(), h->stride, n, (int)order.size() == n ? order.data() : nullptr,
                    (int)start.size() == n ? start.data() : nullptr, spec, t, err))
        return fail(h, SWE2D_ERR_UNSUPPORTED, err);
    return SWE2D_OK;
}

// the device records of a table: int2 {cell, w0 | w1 << 10 | w2 << 20}; with four facets int4 {cell, w0..2, w3, 0}
std::vector<int> tile_records(const TileTable &t, int nfacets)
{
    std::vector<int> rec;
    for (size_t i = 0; i < t.cell.size(); i++) {
        const unsigned *w = &t.facet[i*nfacets];
        rec.push_back(t.cell[i]);
        rec.push_back((int)(w[0] | (w[1] << SWE_FUSE_FBITS) | (w[2] << (2*SWE_FUSE_FBITS))));
        if (nfacets == 4) { rec.push_back((int)w[3]); rec.push_back(0); }
    }
    return rec;
}

// allocations and copies: never inside a stream capture (the callers test).  lane_slot: the three-stage kernel's third plane of lane
// records, the staging slot each lane gathers (the stage pairs gather by lane and facet and have none)
int upload_tiles(Handle *h, TileSet &ts, const std::vector<int> &rec, const std::vector<int> &counts, const TileTable &t,
                 const std::vector<unsigned> *lane_slot = nullptr)
{
    HIP_TRY(h, ts.tile.alloc(rec.size()));
    HIP_TRY(h, ts.counts.alloc(counts.size()));
    HIP_TRY(h, hipMemcpy(ts.tile, rec.data(), rec.size()*sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(ts.counts, counts.data(), counts.size()*sizeof(int), hipMemcpyHostToDevice));
    if (lane_slot) {
        HIP_TRY(h, ts.lane_slot.alloc(lane_slot->size()));
        HIP_TRY(h, hipMemcpy(ts.lane_slot, lane_slot->data(), lane_slot->size()*sizeof(unsigned), hipMemcpyHostToDevice));
    }
    ts.n_tiles = (int)t.n_inner.size();
    ts.ring[0] = t.ring[0]; ts.ring[1] = t.ring[1];
    return SWE2D_OK;
}
}  // namespace

// the stage pair's tables (triangles or quadrilaterals).  Not inside a stream capture - such a capture keeps the stage launches, the
// next call outside one builds
int fuse12_build(Handle *h)
{
    TileSet &ts = pair_tiles(h);
    if (ts.tile || h->fuse_state == -1 || stream_capturing(h)) return SWE2D_OK;
    TileTable t;
    if (int rc = build_table(h, h->npc == 4 ? kQuadPairTiles : kPairTiles, h->fuse_order, {}, t)) return rc;
    if (!fuse12_tiles_pay(h, (int)t.n_inner.size())) { h->fuse_state = -1; return SWE2D_OK; }
    return upload_tiles(h, ts, tile_records(t, h->npc), t.n_inner, t);
}

// stages 1 and 2 of a step: state buffer A (U(0)) -> state buffer C (U(2)) on the cells [0, cell_end); stage 3 follows as a stage launch
template <class Args>
static int launch_pair(Handle *h, void (*kern)(const Args), int cell_end)
{
    const TileSet &ts = pair_tiles(h);
    if (!ts.tile) return fail(h, SWE2D_ERR_UNSUPPORTED, "fused stage pair: no tile tables");     // (step_ready builds them)
    Args q;
    fill_stage_args(h, q.st, 0, 0, 2, 0.0, 1.0, kBeta[0], 0, h->n_owned);
    q.st.idxc = h->opt[SWE2D_OPT_COMPACT_IDX] == 0 ? nullptr : h->idxc;      // (the 16-B connectivity records: a streaming kernel; triangles only)
    q.tile = reinterpret_cast<decltype(q.tile)>(ts.tile.get());
    q.n_inner = ts.counts;
    q.n_tiles = ts.n_tiles;
    q.cell_end = cell_end;
    q.beta1 = kBeta[0];
    q.a0_2 = kAlpha0[1]; q.a1_2 = kAlphaIn[1]; q.beta2 = kBeta[1];
    q.out = h->state[2];
    const int grid = ((ts.n_tiles + 7)/8)*8;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SWE_FUSE_WG), 0, h->stream, q);
    HIP_TRY(h, hipGetLastError());
    stage_written(h, false, true);                          // U(1) never left the chip; buffer C holds U(2)
    return SWE2D_OK;
}

int launch_fuse12(Handle *h, int cell_end)
{
    const bool nl = h->par.use_nonlinear_equations != 0, lf = h->par.use_lax_friedrichs_velocity != 0;
    if (h->npc == 4)
        return launch_pair(h, pick_instance([](auto a, auto b, auto c, auto d) -> void (*)(const SweFuseQuadArgs) {
                               return swe_fuse12_quad_kernel<a.value, b.value, c.value, d.value>; }, nl, lf, has_sources(h), h->affine), cell_end);
    return launch_pair(h, pick_instance([](auto a, auto b, auto c) -> void (*)(const SweFuseArgs) {
                           return swe_fuse12_kernel<a.value, b.value, c.value>; }, nl, lf, has_sources(h)), cell_end);
}

// all three stages in one launch (swe_fuse123_kernel): tiles with two rings, in the order of swe2d_fused_set_triple_tiles if there is
// one.  Not inside a stream capture - there it builds nothing (fuse3.tile stays null) and the caller goes without.
int fuse123_build(Handle *h)
{
    if (h->fuse3.tile || stream_capturing(h)) return SWE2D_OK;
    TileTable t;
    if (int rc = build_table(h, kTripleTiles, (int)h->fuse3_order.size() == h->n_cells ? h->fuse3_order : h->fuse_order, h->fuse3_start, t)) return rc;
    std::vector<int> counts;                                // int2 {n_inner, n_mid | rot << 16}
    for (size_t i = 0; i < t.n_inner.size(); i++) { counts.push_back(t.n_inner[i]); counts.push_back(t.n_mid[i] | (t.rot[i] << 16)); }
    // the lanes' and the slots' records, decoded here once per table (swe2d_tiles.h: build_lane_records): the kernel reads no connectivity
    LaneRecords r;
    build_lane_records(t, h->h_nbr.data(), h->h_cv.data(), h->stride, SWE_FUSE_WG, 8u*SWE_FUSE3_XG, (unsigned)h->stride*8u, r,
                       SWE_FUSE3_STAGING_PLANES ? kStagingPlanes : kStagingSlot6);
    return upload_tiles(h, h->fuse3, r.lane, counts, t, &r.lane_slot);
}

// a whole step: state buffer A (U(0)) -> state buffer B (U(3)), then the two change places
int launch_fuse123(Handle *h, int cell_end)
{
    if (int rc = capture_parity_check(h)) return rc;          // (an earlier capture's count is settled before this launch swaps)
    if (int rc = fuse123_build(h)) return rc;
    if (!h->fuse3.tile) return fail(h, SWE2D_ERR_UNSUPPORTED, "fused stages: no tile tables (not built inside a stream capture)");
    SweFuse3Args q;
    fill_stage_args(h, q.st, 0, 0, 1, 0.0, 1.0, kBeta[0], 0, h->n_owned);
    q.rec = reinterpret_cast<const int4 *>(h->fuse3.tile.get());
    q.counts = reinterpret_cast<const int2 *>(h->fuse3.counts.get());
    q.lane_slot = reinterpret_cast<const uint2 *>(h->fuse3.lane_slot.get());
    q.n_tiles = h->fuse3.n_tiles;
    q.cell_end = cell_end;
    for (int s = 0; s < 3; s++) { q.a0[s] = s ? kAlpha0[s] : 0.0; q.a1[s] = s ? kAlphaIn[s] : 1.0; q.beta[s] = kBeta[s]; }
    q.out = h->state[1];
    auto kern = pick_instance([](auto a, auto b, auto c) -> void (*)(const SweFuse3Args) { return swe_fuse123_kernel<a.value, b.value, c.value>; },
                              h->par.use_nonlinear_equations != 0, h->par.use_lax_friedrichs_velocity != 0, has_sources(h));
    const int grid = ((h->fuse3.n_tiles + 7)/8)*8;
    SWE_CHK_SYNC(h->stream);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SWE_FUSE_WG), 0, h->stream, q);
    HIP_TRY(h, hipGetLastError());
    swap_state_buffers(h);                                  // (U(1) and U(2) never left the chip)
    // inside a stream capture the swap is only the host's: a graph that holds an odd number of them ends on the other buffer than it
    // began on and cannot be replayed twice - counted per capture here, reported by capture_parity_check at the next call outside it
    unsigned long long id = 0;
    if (stream_capturing(h, &id)) {
        if (id != h->capture_id) { h->capture_id = id; h->capture_swaps = 0; }   // (an earlier capture's count was settled above)
        h->capture_swaps++;
    }
    return SWE2D_OK;
}

// Called on entry by every function that reads or writes the state buffers.  Once the capture that swapped has ended (no capture, or
// another one) an odd count is settled: the host swap is undone - nothing ran, buffer A still holds the state from before the capture -
// and the next call outside a capture returns SWE2D_ERR_UNSUPPORTED, once, without doing anything.
int capture_parity_check(Handle *h)
{
    if (h->capture_swaps == 0 && h->capture_odd == 0) return SWE2D_OK;
    unsigned long long id = 0;
    const bool capturing = stream_capturing(h, &id);
    if (h->capture_swaps) {
        if (capturing && id == h->capture_id) return SWE2D_OK;
        if (h->capture_swaps & 1) { swap_state_buffers(h); h->capture_odd++; }
        h->capture_swaps = 0;
    }
    if (capturing || h->capture_odd == 0) return SWE2D_OK;
    const int odd = h->capture_odd;
    h->capture_odd = 0;
    return fail(h, SWE2D_ERR_UNSUPPORTED, std::to_string(odd) + " stream capture(s) recorded an odd number of swe2d_solve_step_cells launches: "
                "such a graph ends on the other state buffer than it began on and cannot be replayed (the state is the one from before the "
                "capture); capture an even number per sequence");
}

}  // namespace swe2d_impl

// a tile order handed in by the caller (null: none): a permutation of the cells
static int checked_tile_order(Handle *h, const int32_t *cells, std::vector<int> &order)
{
    std::vector<char> seen((size_t)h->n_cells, 0);
    for (int i = 0; cells && i < h->n_cells; i++) {
        if (cells[i] < 0 || cells[i] >= h->n_cells || seen[cells[i]]) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "fused stages: the tile order is not a permutation of the cells");
        seen[cells[i]] = 1;
    }
    if (cells) order.assign(cells, cells + h->n_cells);
    return SWE2D_OK;
}

extern "C" {

int swe2d_fused_set_order(swe2d_handle *hh, const int32_t *cells_in_tile_order)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<int> order;
    if (int rc = checked_tile_order(h, cells_in_tile_order, order)) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (TileSet *ts : {&h->fuse, &h->fuseq, &h->fuse3}) *ts = TileSet();
    if (h->fuse_state == -1) h->fuse_state = 0;
    h->fuse_order.swap(order);
    return SWE2D_OK;
}

int swe2d_fused_set_triple_tiles(swe2d_handle *hh, const int32_t *cells_in_tile_order, const int32_t *tile_starts, int32_t n_starts)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<int> order;
    std::vector<unsigned char> start;
    if (int rc = checked_tile_order(h, cells_in_tile_order, order)) return rc;
    if (n_starts < 0 || (n_starts > 0 && !tile_starts)) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "fused stages: tile starts");
    if (n_starts > 0) {
        start.assign((size_t)h->n_cells, 0);
        for (int i = 0; i < n_starts; i++) {
            if (tile_starts[i] < 0 || tile_starts[i] >= h->n_cells) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "fused stages: a tile start outside the cells");
            start[tile_starts[i]] = 1;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->fuse3 = TileSet();
    h->fuse3_order.swap(order);
    h->fuse3_start.swap(start);
    return SWE2D_OK;
}

// out[0] = 1 when `who` takes the three-stage kernel now (builds the tile tables; inside a stream capture nothing is built and the
// answer is 0 while they are missing: the caller takes the stage launches), out[1] = tiles, out[2] / out[3] = cells of the two rings
static int fused_triple_info(Handle *h, StepCaller who, int32_t out[4])
{
    if (!h || !out) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    StepPath path;
    if (int rc = step_ready(h, who, kTriple, &path)) return rc;
    if (path != kTriple) return SWE2D_OK;
    out[0] = 1; out[1] = h->fuse3.n_tiles; out[2] = (int32_t)h->fuse3.ring[0]; out[3] = (int32_t)h->fuse3.ring[1];
    return SWE2D_OK;
}
int swe2d_fused_triple_info(swe2d_handle *hh, int32_t out[4]) { return fused_triple_info(H(hh), kWholeStep, out); }
// by itself where the caller handed in patches (swe2d_fused_set_triple_tiles) and the cell range is beyond the dataflow kernel's
int swe2d_fused_step_info(swe2d_handle *hh, int32_t out[4]) { return fused_triple_info(H(hh), kPartitionStep, out); }

// All three stages of a step on a partition: stage 3 on [0, cell_end) - the last of the step's three shrinking ranges; the tiles
// evaluate stages 1 and 2 on supersets of theirs (every cell of a tile / interior + first ring), values that never leave the chip.
// U(3) goes to state buffer B and the two change places: cells of the new buffer A beyond cell_end hold what B held before - stale
// ghost values that the next exchange rewrites, and that no later stage of the cycle reads (its ranges end inside cell_end).
int swe2d_solve_step_cells(swe2d_handle *hh, int32_t cell_end)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (cell_end < 0 || cell_end > h->n_cells) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "bad cell range");
    // (the caller's launch: whatever the size - swe2d_fused_step_info holds the rule)
    if (!(step_kernels(h) & kTriple)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_solve_step_cells: the three-stage kernel does not cover this handle");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = capture_parity_check(h)) return rc;
    if (!h->fuse3.tile && stream_capturing(h))    // tile tables: allocations and copies, not inside a stream capture
        return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_solve_step_cells: first call inside a stream capture (swe2d_fused_step_info builds the tables)");
    return launch_fuse123(h, cell_end);
}

// stages 0 and 1 of a step on the ranges [0, cell_end_0) and [0, cell_end_1) (cell_end_1 <= cell_end_0, every cell of the second
// range with its facet neighbours inside the first: a partition's stage ranges): one fused launch where the kernel covers the
// handle, else the two stage launches.  Buffer C holds U(2) on [0, cell_end_1) afterwards either way.
int swe2d_solve_stage_pair_cells(swe2d_handle *hh, int32_t cell_end_0, int32_t cell_end_1)
{
    Handle *h = H(hh);
    if (!h) return SWE2D_ERR_INVALID_ARGUMENT;
    if (cell_end_1 < 0 || cell_end_1 > cell_end_0 || cell_end_0 > h->n_cells) return fail(h, SWE2D_ERR_INVALID_ARGUMENT, "bad cell ranges");
    // (two stages in one call: the second would see the boundary elevation / the atmospheric fields of the first stage's time)
    if (forced(h)) return fail(h, SWE2D_ERR_UNSUPPORTED, "swe2d_solve_stage_pair_cells: not with a tide table or an atmospheric record (swe2d_tide_eval / swe2d_atm_eval + swe2d_solve_stage_cells per stage)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = capture_parity_check(h)) return rc;
    StepPath path;
    if (int rc = step_ready(h, kPartitionPair, kPair, &path)) return rc;
    if (path == kPair) return launch_fuse12(h, cell_end_1);
    if (int rc = stage_on_range(h, 0, 0, cell_end_0)) return rc;
    return stage_on_range(h, 1, 0, cell_end_1);
}

#ifdef SWE_WAVE_TIMING
// profiling build only (tools/fuse3_phases.py): the phase stamps of the LAST three-stage launch, n_wg sampled workgroups x 4 waves x
// SWE_F3P_WORDS words (swe2d_fuse.h); out[0..2] of info = words per wave, stamps per wave, the most workgroups the buffer samples
int swe2d_debug_read_fuse3_phases(swe2d_handle *hh, unsigned long long *out, int32_t n_wg, int32_t info[3])
{
    Handle *h = H(hh);
    if (!h || !info || n_wg < 0 || n_wg > SWE_F3P_MAX_WG) return SWE2D_ERR_INVALID_ARGUMENT;
    info[0] = SWE_F3P_WORDS; info[1] = SWE_F3P_STAMPS; info[2] = SWE_F3P_MAX_WG;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (n_wg > 0) HIP_TRY(h, hipMemcpyFromSymbol(out, HIP_SYMBOL(swe_fuse3_phase), sizeof(unsigned long long)*4*SWE_F3P_WORDS*(size_t)n_wg));
    return SWE2D_OK;
}
#endif

}  // extern "C"
