// swe2d_handle.h - what the translation units of the C ABI share: the handle, error plumbing, internal entry points.
// Not part of the boundary (include/swe2d.h is).
#pragma once
#include "../../include/swe2d.h"
#include "swe2d_kernels.h"
#include "swe2d_sipg.h"
#include "swe2d_flow.h"
#include "swe2d_p2p.h"
#include "swe2d_devmem.h"

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <atomic>
#include <map>
#include <mutex>

static_assert(SWE2D_MAX_MARKERS == SWE_MAX_MARKERS, "marker table size mismatch");
static_assert(SWE2D_MAX_FARMS == SWE_MAX_FARMS && SWE2D_MAX_THRUST_TABLE == SWE_MAX_THRUST_TABLE, "turbine farm table size mismatch");

#ifdef SWE_RANGE_CHECK
// Range-checked build (swe2d_kernels.h): every device allocation of this library (swe2d_devmem.h) is recorded with its requested size;
// the sorted table is copied to the device before a launch whenever it changed.
namespace {
std::mutex g_chk_mutex;
std::map<unsigned long long, unsigned long long> g_chk_allocs;       // base -> end
bool g_chk_dirty = true;
unsigned long long g_chk_launches = 0;
void swe_chk_upload_locked()
{
    static SweChkTable t;
    t.n = 0;
    for (auto &kv : g_chk_allocs) if (t.n < SWE_CHK_MAX) { t.lo[t.n] = kv.first; t.hi[t.n] = kv.second; t.n++; }
    (void)hipDeviceSynchronize();
    (void)hipMemcpyToSymbol(HIP_SYMBOL(swe_chk_tab), &t, sizeof(t));
    g_chk_dirty = false;
}
// the funnel's hook (swe_dev_alloc / swe_dev_free, swe2d_api.hip)
void swe_chk_record(void *p, size_t n)
{
    std::lock_guard<std::mutex> lock(g_chk_mutex);
    const char *st = getenv("THETIS_AMD_RANGE_SELFTEST");                  // negative control: record half of every allocation
    g_chk_allocs[(unsigned long long)p] = (unsigned long long)p + ((st && atoi(st)) ? n/2 : n);
    // the table goes to the device now: the next checked launch may be recorded in a stream capture, where it cannot be
    // copied, and the replays would check against a table without this allocation (the library never allocates inside one)
    swe_chk_upload_locked();
}
void swe_chk_forget(void *p)
{
    std::lock_guard<std::mutex> lock(g_chk_mutex);
    g_chk_allocs.erase((unsigned long long)p);
    g_chk_dirty = true;
}
void swe_chk_sync(hipStream_t stream)
{
    std::lock_guard<std::mutex> lock(g_chk_mutex);
    g_chk_launches++;
    if (!g_chk_dirty) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return;
    swe_chk_upload_locked();
}
}
#define SWE_CHK_SYNC(stream) swe_chk_sync(stream)
extern "C" int swe2d_debug_range_report(unsigned long long out[5])
{
    std::lock_guard<std::mutex> lock(g_chk_mutex);
    (void)hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(swe_chk_report), 4*sizeof(unsigned long long)) != hipSuccess) return 1;
    out[3] = g_chk_launches;
    out[4] = g_chk_allocs.size();
    return 0;
}
#else
#define SWE_CHK_SYNC(stream) ((void)0)
#endif

namespace swe2d_impl {

extern thread_local std::string g_create_error;

// Shu-Osher coefficients of SSPRK33 (swe2d_api.hip)
extern const double kBeta[3], kAlpha0[3], kAlphaIn[3];

extern std::atomic<unsigned long long> g_next_uid;

// the tile tables of one fused kernel on the device (swe2d_api_fuse.hip: upload_tiles); tile empty: not built
struct TileSet {
    DevArray<int> tile;                                 // [n_tiles][256] records: int2, quadrilaterals int4 (SweFuseArgs / SweFuseQuadArgs); two-ring
                                                        // tiles: [n_tiles][2][256] int4, the decoded lane records (SweFuse3Args::rec)
    DevArray<int> counts;                               // [n_tiles] n_inner; two-ring tiles: int2 {n_inner, n_mid | rot << 16}
    DevArray<unsigned> lane_slot;                       // two-ring tiles only: [n_tiles][256] uint2, per lane the decoded byte offsets of the
                                                        // staging slot it gathers, or {~0u, ~0u} (SweFuse3Args::lane_slot)
    int n_tiles = 0;
    long long ring[2] = {0, 0};                         // cells of ring 1 / ring 2 over all tiles
};

struct Handle {
    unsigned long long uid = g_next_uid.fetch_add(1ull);   // never reused (a freed handle's address may be)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t my_stream = nullptr;
    hipStream_t xstream = nullptr;                     // the exchange kernels' stream (swe2d_set_exchange_stream), null: `stream`
    int n_cells = 0, n_owned = 0, n_interior = 0, n_vertices = 0;
    int npc = 3;                                       // nodes per cell: 3 triangles, 4 quadrilaterals
    bool affine = true;                                // quadrilaterals: every cell a parallelogram (constant Jacobian, tensor mass inverse)
    bool affine_local = true;                          // ... as found in this handle's own cells (affine may be forced off: swe2d_set_general_quadrilaterals)
    size_t stride = 0;
    DevArray<double> state[3];                        // A (U0 / step result), B (U1), C (U2)
    DevArray<int> nbr, cv;
    // compact boundary uploads (swe2d_set_bc_facets): the (cell, facet) lists of the last calls stay on the device, a repeated
    // call with the same lists (update_forcings at every stage) only uploads the values
    struct FacetList { std::vector<int32_t> cells, facets; DevArray<int> dev; };
    FacetList facet_lists[8];
    int facet_list_next = 0;
    DevArray<int4> opp4;                                // triangles: opposite vertices of the neighbours (fused viscosity)
    DevArray<int> bnd_cells;                            // cells with a boundary facet (boundary-only SIPG launch)
    int n_bnd = 0;
    int opt[SWE2D_OPT_COUNT];                           // swe2d_set_option: -1 = the library's own rule (set in the constructor below)
    Handle() { for (int i = 0; i < SWE2D_OPT_COUNT; i++) opt[i] = -1; }
    // which of the stage buffers hold the stage solutions of the step made last (swe2d_get_stage_state): the fused and the dataflow
    // kernels keep U(1) (and U(2)) on chip
    // (a launch inside a stream capture runs nothing: it clears both, see stage_written)
    bool stage_valid[2] = {false, false};
    // buffer swaps made while the stream was capturing (launch_fuse123): must be even per captured sequence.  Counted per capture
    // (capture_id, the id hipStreamGetCaptureInfo gives); a capture that ended on an odd count has its host swap undone and is
    // counted in capture_odd until capture_parity_check reports it outside a capture
    int capture_swaps = 0;
    unsigned long long capture_id = 0;
    int capture_odd = 0;
    DevArray<int4> idx4;                                // packed triangle connectivity (stage kernel), see SweStageArgs
    DevArray<int2> idx2;
    DevArray<int4> idxc;                                // ... in 16 B (swe_conn_pack), what the stage kernels read (SWE2D_OPT_COMPACT_IDX)
    // tile tables of the fused stage kernels (swe2d_fuse.h; SWE2D_OPT_FUSED_STAGES), built at first use (swe2d_tiles.h): the stage pair
    // on triangles (swe_fuse12_kernel), on quadrilaterals (swe_fuse12_quad_kernel), all three stages with two rings per tile
    // (swe_fuse123_kernel)
    TileSet fuse, fuseq, fuse3;
    int fuse_state = 0;                                 // -1: the numbering gives poor tiles (stage launches until an option or the order changes)
    std::vector<int> fuse_order;                        // cells in the order the tiles are cut from (swe2d_fused_set_order); empty: the numbering
    std::vector<int> fuse3_order;                       // the same for the two-ring tiles alone (swe2d_fused_set_triple_tiles); empty: fuse_order
    std::vector<unsigned char> fuse3_start;             // [n_cells] 1 = a two-ring tile must begin at this position of the order; empty: none
    int n_conn_escapes = 0;                             // cells whose record is an escape to the wide ones
    std::vector<int> h_nbr;                             // host copy of the packed neighbour codes [3][S] (triangles; flow_build)
    std::vector<int> h_cv;                              // host copy of the vertex ids [3][S] (triangles: the lane records of the two-ring tiles)
    // dataflow stage loop (swe2d_flow.h): per-block stage counters, status word {timeouts, first late block + 1}
    DevArray<unsigned> flow_flag, flow_status;
    DevArray<int4> flow_xo4;                            // exchange slots of the rim facets (facets between two 64-cell blocks), see SweFlowArgs
    DevArray<int2> flow_xo2;
    DevArray<int2> flow_xblk;
    DevArray<int> flow_xsrc;
    std::vector<int> h_send, h_recv;                    // host copies of the halo lists (swe2d_halo_setup)
    std::vector<int> flow_fpos;                         // cell -> flow position
    DevArray<int2> flow_xsend;                          // FX: per position, the cell's places in the send list
    DevArray<int> flow_xrecv;                           // FX: per position, the cell's place in the receive list
    DevArray<unsigned> flow_xtick;
    int flow_push_blocks = 0, flow_recv_blocks = 0;
    bool flow_x_ready = false;                          // the FX tables match the halo lists and the flow order
    DevArray<int> flow_cell;                            // [flow_blocks*64] flow position -> cell (< 0: padding lane, -1 - cell to mimic)
    unsigned flow_parity_bytes = 0;
    DevArray<char> flow_ex;
    size_t flow_ex_bytes = 0;
    int flow_blocks = 0;                                // 64-cell blocks of the handle
    int flow_capacity = -1;                             // resident one-wave workgroups of the flow kernel on this device (-1: not asked yet)
    int flow_max_rim = 0;                               // most rim facets of a block in the current flow order (selects the polling width)
    int launch_parity = 0;                              // direction of the next large stage launch (launch_stage)
    bool flow_used = false;                             // a flow launch since the status word was last read
    DevArray<double> vx, vy, vh;
    DevArray<double> bc_field[4];                                // Function-valued boundary data per facet: elev, uv, un, flux
    DevArray<double> valpha;                           // per-vertex wetting-drying alpha
    bool wd = false;
    bool state_holds_D = false;                        // wetting-drying: the elevation planes of buffer A hold the displaced depth D
    struct Snapshot { DevArray<char> data; bool holds_D = false; };
    Snapshot snapshot[SWE2D_SNAPSHOT_SLOTS];           // swe2d_state_snapshot: buffer A + the tracers' buffers A, per slot
    // SIPG horizontal viscosity (optional pass after each stage kernel)
    bool visc = false;
    DevArray<double> nu_v;                             // per-vertex viscosity or null (constant)
    double nu_const = 0.0, sipg_factor = 1.0;
    int visc_grad_div = 0, visc_grad_depth = 1;
    DevArray<double> field[SWE2D_FIELD_COUNT];
    double scalar[SWE2D_SCALAR_COUNT] = {-1.0, -1.0, -1.0, 0.0, -1.0};
    DevArray<double> stage_uv, stage_eta;              // device staging in host layout (6N + 3N)
    DevArray<double> partial;                          // diagnostics partial sums
    int n_partial_blocks = 0;
    DevArray<unsigned long long> diag_acc;             // limb sums of the diagnostics kernels (swe_sum_accumulate) + one counter
    DevArray<int> send_cells, recv_cells;
    int n_send = 0, n_recv = 0;
    // peer-to-peer halo (swe2d_p2p.h): my landing zone, the peers' zones mapped here, per-channel device counters.  The zone and the
    // mappings stay outside DevArray: the zone is one of three kinds of memory (hipExtMallocWithFlags) that peers hold open by
    // IPC, a mapping is closed and not freed; swe2d_destroy releases both by hand
    struct P2p {
        void *zone = nullptr;
        size_t zone_bytes = 0;
        int zone_kind = 0;                               // 1 uncached, 2 fine-grained, 3 ordinary device memory
        int n_channels = 0;
        int width[SWE_P2P_MAX_CHANNELS] = {0};
        DevArray<SweP2pCounters> ctr;                    // [n_channels]
        std::vector<void *> opened;                      // hipIpcOpenMemHandle mappings to close
        int n_peers = 0, n_from = 0;
        int off[SWE_P2P_MAX_PEERS], cnt[SWE_P2P_MAX_PEERS], remote_off[SWE_P2P_MAX_PEERS], remote_flag[SWE_P2P_MAX_PEERS],
            remote_n_recv[SWE_P2P_MAX_PEERS];
        char *remote_base[SWE_P2P_MAX_PEERS];
    } p2p;
    // tracers + limiter
    struct Tracer {
        DevArray<double> buf[3];                        // A (T0 / result), B, C: 3 planes each
        DevArray<double> source;
        bool conservative = false;                      // options.tracer[label].use_conservative_form
        DevArray<double> bc_value_f;                    // Function-valued 'value' boundaries, npc*npc planes
        int bc_vel_kind[SWE_MAX_MARKERS];               // 0 none, 1 'uv', 2 'un'
        double bc_u[SWE_MAX_MARKERS], bc_v[SWE_MAX_MARKERS];
        DevArray<double> bc_vel_f;                      // Function-valued 'uv' / 'un' / 'flux', 4*npc planes per facet layout
        int bc_vel_field[SWE_MAX_MARKERS];
        int bc_has_value[SWE_MAX_MARKERS];
        double bc_value[SWE_MAX_MARKERS];
        bool diff = false;                              // SIPG horizontal diffusion
        DevArray<double> mu_v;
        double mu_const = 0.0, sipg_factor = 1.0;
        int bc_diff_kind[SWE_MAX_MARKERS];
        double bc_diff_flux[SWE_MAX_MARKERS];
        // reaction program (swe2d_reaction.hip): n_code > 0 = a pass in front of every stage launch writes `source`
        struct Reaction {
            int n_code = 0, n_const = 0, n_q = 0, n_tracers = 0;
            int code[SWE2D_REACTION_MAX_CODE] = {0};            // as launched: the arg of TRACER / FIELD is a slot of the operand table
            double consts[SWE2D_REACTION_MAX_CONSTS] = {0.0};
            int tracer_ids[SWE2D_REACTION_MAX_TRACERS] = {0};   // operand slot -> tracer id
            unsigned field_mask = 0u;                           // coefficient slots the program names
            double phi[SWE2D_REACTION_MAX_QUAD*4] = {0.0}, w[SWE2D_REACTION_MAX_QUAD] = {0.0};
        };
        Reaction rx;
    };
    std::vector<Tracer> tracers;
    DevArray<double> rx_field[SWE2D_REACTION_MAX_FIELDS];                                 // coefficient fields of the reaction programs, npc planes
    // suspended sediment + Exner (swe2d_sediment.hip): on = tracer `tracer` is the sediment field, its source comes from `planes`
    struct Sediment {
        bool on = false;
        int tracer = -1;
        swe2d_sediment_params par{};
        DevArray<double> planes;                        // E | D | equilibrium, 3 nodal planes each (swe2d_sediment_update)
        unsigned eq_markers = 0u;                       // bit m: marker slot m carries 'equilibrium'
    };
    Sediment sed;
    // what the sediment field, the bedload model and the slide share (swe2d_sediment.hip): built by the first of them that needs
    // it (exner_tables_build, gradient_table_build), released by exner_release_unused when the last one that reads it is switched off
    struct Exner {
        DevArray<int> v_off, v_ent;                     // vertex -> (cell << 2 | local node), cells ascending (the Exner gather)
        DevArray<double> area;                          // [n_cells]
        DevArray<double> vh_new;                        // [n_vertices] the Exner kernel's output, copied over vh
        DevArray<unsigned> count;                       // vertices an Exner update left unchanged (depth below the floor)
    };
    Exner exner;                                        // read by all three
    DevArray<double> exner_grad;                        // d psi_i/dx [3][S] | d psi_i/dy [3][S], built on the host: read by the bedload model and the slide
    // bedload transport in the Exner update (swe2d_sediment.hip), with or without a sediment field
    struct Bedload {
        bool on = false;
        swe2d_bedload_params par{};
        DevArray<double> planes;                        // qbx [3][S] | qby [3][S] | contribution [3][S] (swe2d_bedload_update)
    };
    Bedload bed;
    // sediment slide in the Exner update (swe2d_sediment.hip)
    struct Slide {
        bool on = false;
        swe2d_slide_params par{};
        DevArray<double> planes;                        // alpha [S] | beta [S] | contribution [3][S] (swe2d_slide_update)
        DevArray<double> region;                        // [n_cells] slide region per cell; null: 1 everywhere
        DevArray<unsigned long long> words;             // [0] bits of the largest beta of the last pass, [1] flagged cells since set
    };
    Slide slide;
    // Smagorinsky eddy viscosity (swe2d_smag.hip): on = nu_v is rewritten in front of every step, the caller's viscosity is the background
    struct Smag {
        bool on = false;
        bool visc_caller = false;                       // the caller's own viscosity switch (swe2d_set_viscosity), restored by swe2d_smag_clear
        double cs = 0.0, min_val = 0.0, max_const = -1.0;
        DevArray<double> bg_v;                          // [n_vertices] the caller's per-vertex viscosity, or null: bg_const
        double bg_const = 0.0;
        DevArray<double> he;                            // [n_vertices] element size
        DevArray<int> off, ent;                         // vertex -> (cell << 2 | local node), in the caller's order
        DevArray<double> planes;                        // b_0 b_1 b_2 | A/3, [stride] each (the cell pass)
        DevArray<double> nu_clip;                       // [n_vertices] the clipped closure viscosity (the vertex pass)
        DevArray<double> grad, grad_out;                // debug: 12 gradient planes and their staging, allocated by the first read
    };
    Smag smag;
    int tracer_use_lf = 0;
    double tracer_lf_factor = 1.0, tracer_vel_factor = 1.0;
    std::vector<int> host_cells;                 // [n][3] vertex ids as given (limiter default topology)
    std::vector<int> host_nbr;                   // [n][3]
    int lim_nv = 0;
    DevArray<int> lim_v2c_off, lim_v2c_cell, lim_vbf_off, lim_vbf_facet, lim_tv;
    DevArray<double> lim_mean, lim_qmin, lim_qmax;
    // point probes (swe2d_probe.hip): slot = probe id; a destroyed set leaves an empty slot
    struct Probe {
        bool live = false;
        int n_points = 0, width = 0, capacity = 0, rows = 0;
        DevArray<int> cell;                             // [n_points] device cells
        DevArray<double> weight;                        // [n_points][npc]
        DevArray<double> out;                           // [capacity + 1][n_points][width]: the last row is swe2d_probe_eval's
        std::vector<int> fields;                        // SWE2D_PROBE_UV / SWE2D_PROBE_ELEV / tracer id
    };
    std::vector<Probe> probes;
    // tidal turbine farms (swe2d_turbine.hip): slot = farm id
    struct Farm {
        bool live = false;
        swe2d_turbine_params par{};
        DevArray<double> density;                       // npc nodal planes, zero outside the farm's cells
        DevArray<int> cells;                            // owned cells with a non-zero density
        int n_list = 0;
        // a discrete farm (swe2d_dfarm.hip): single turbines as bump densities, tabulated at the points of the farm's own rule over
        // `cells` - here the owned cells of the subdomain whose bounding box meets a turbine's square.  `density` stays null.
        bool discrete = false;
        int n_q = 0, n_turbines = 0;                    // points of the rule, turbines
        double radius = 0.0;                            // projected_diameter / 2
        DevArray<double> dtab;                          // [n_q][n_list] density at the points of the listed cells
        DevArray<double> txy;                           // [n_turbines][2] turbine coordinates
        DevArray<int> csr;                              // c_off [n_list + 1] | c_idx [nnz] | t_off [n_turbines + 1] | t_pos [nnz]
        int nnz = 0;                                    // (cell, candidate turbine) pairs
        DevArray<unsigned long long> tpow;              // [n_turbines][SWE_SUM_LIMBS + 1] limb sums of swe2d_dfarm_turbine_power
        double phi[SWE2D_MAX_FARM_QUAD*4] = {0.0}, w[SWE2D_MAX_FARM_QUAD] = {0.0};     // the rule (kernel arguments of the passes)
    };
    Farm farms[SWE2D_MAX_FARMS];
    int n_farms = 0;                                    // live slots
    int n_cfarms = 0;                                   // ... of them continuous: the ones the stage kernels carry (SweStageArgs::farms)
    DevArray<SweFarmTable> farm_table;                  // the device's copy of the farms' constants (SweStageArgs::farms)
    int farm_blocks = 0;                                // blocks of a power launch
    DevArray<unsigned long long> farm_rows;             // [farm_rows_cap + 1][SWE_FARM_ROW] limb sums; the last row is swe2d_turbine_power's
    int farm_rows_cap = 0, farm_rows_n = 0;
    // harmonic tidal boundary elevation (swe2d_tide.hip): n > 0 = the handle has a tide table
    struct Tide {
        int n = 0, K = 0;                               // boundary facets, constituents
        double omega[SWE2D_MAX_TIDE_CONSTITUENTS] = {0.0};
        DevArray<double> tab;                           // mean [2n] | amp [K][2n] | phase [K][2n]
        DevArray<int> list;                             // device cells [n] | facets [n]
        DevArray<double> out;                           // [2n] staging of swe2d_tide_read
    };
    Tide tide;
    // atmospheric forcing (swe2d_atm.hip): n_t > 0 = the handle has a record of wind / pressure snapshots
    struct Atm {
        int n_t = 0, which = 0, method = 0, W = 0;      // snapshots, quantities (wind = 1 | pressure = 2), stress formulation, doubles per vertex
        std::vector<double> times;                      // [n_t] the host's copy: the bracket of a time is found here (atm_launch)
        DevArray<double> tab;                           // [n_t][n_vertices][W]: u, v | p | u, v, p of a vertex interleaved
    };
    Atm atm;
    // the clock of the forcings (swe2d_tide_clock): step k of the next advance starts at clock_t_base + (clock_k_first + k)*dt
    double clock_t_base = 0.0;
    long long clock_k_first = 0;
    // running field statistics (swe2d_stats.hip): slot = statistics id; a destroyed set leaves an empty slot
    struct Stats {
        bool live = false;
        int K = 0;                                      // harmonic constituents
        DevArray<double> acc;                           // [8 + 2K][npc][stride] accumulator planes, laid out like the state
        long long n_samples = 0;                        // appends since create / reset
    };
    std::vector<Stats> stats;
    // Lagrangian particles (swe2d_particles.hip): slot = particle set id; a destroyed set leaves an empty slot
    struct Particles {
        bool live = false;
        int n = 0, capacity = 0, rows = 0;
        DevArray<double> pos;                           // [n][2] x, y
        DevArray<int> ist;                              // cell [n] | status [n] | exit marker [n] | wall hits [n]
        DevArray<double> out;                           // [capacity][n][2] recorded positions
        DevArray<double> release;                       // [n] release times (swe2d_particles_set_release_times), else null
        DevArray<double> kv;                            // [n_vertices] diffusivity (swe2d_particles_set_diffusivity), else null
        DevArray<int> counts;                           // [n_cells] of swe2d_particles_cell_counts, allocated at its first call
        unsigned long long seed = 0;                    // the Philox key of the random walk
        unsigned moves = 0;                             // swe2d_particles_advance_at calls so far: the second counter word
    };
    std::vector<Particles> particles;
    // section transports (swe2d_sections.hip): n_lanes > 0 = the handle has sections
    struct Sections {
        int n_lanes = 0;                                // lanes of a launch: every section's pieces padded to whole workgroups
        int n_tracers = 0;
        int tracer_ids[SWE2D_MAX_SECTION_TRACERS] = {0};
        int block0[SWE2D_MAX_SECTIONS + 1] = {0};       // first workgroup of every section slot (block0[s + 1] - block0[s] = its workgroups)
        DevArray<int> cell;                             // [n_lanes] device cell, -1: padding
        DevArray<double> geom;                          // [2*npc + 3][n_lanes]: w[0][.], w[1][.], Nx, Ny, L
        DevArray<unsigned long long> rows;              // [rows_cap + 1][SWE_SECTION_ROW] limb sums; the last row is swe2d_sections_eval's
        int rows_cap = 0, rows_n = 0;
    };
    Sections sections;
    swe2d_params par{};
    SweBcTable bc{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;            // (events and streams: the runtime's objects, destroyed by swe2d_destroy after the arrays)
    std::string err;
};

inline Handle *H(swe2d_handle *h) { return reinterpret_cast<Handle *>(h); }
inline const Handle *H(const swe2d_handle *h) { return reinterpret_cast<const Handle *>(h); }

int fail(Handle *h, int code, const std::string &msg);

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            /* the error is reported through the return code; left in the runtime's "last error" it would surface in the NEXT  \
               caller that checks it - e.g. torch's launch check after a peer mapping that failed (first contact with a node) */ \
            (void)hipGetLastError();                                                             \
            return fail(h, SWE2D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
        }                                                                                        \
    } while (0)

// Optional ROCTx ranges around the entry points that advance the state (SWE2D_OPT_ROCTX = 1): they show up as named ranges in
// `rocprofv3 --marker-trace` next to the kernel trace.  The tracing library is looked up at run time (rocprofiler-sdk's
// librocprofiler-sdk-roctx.so, else roctracer's libroctx64.so) when the first handle asks for it; without it, or without the
// option, the ranges are no-ops.
struct RoctxRange {
    typedef int (*push_t)(const char *);
    typedef int (*pop_t)();
    static void resolve(push_t &push, pop_t &pop)
    {
        static bool done = false;
        static push_t p_push = nullptr;
        static pop_t p_pop = nullptr;
        if (!done) {
            done = true;
            {
                for (const char *name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
                    if (void *lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                        p_push = reinterpret_cast<push_t>(dlsym(lib, "roctxRangePushA"));
                        p_pop = reinterpret_cast<pop_t>(dlsym(lib, "roctxRangePop"));
                        if (p_push && p_pop) break;
                        p_push = nullptr; p_pop = nullptr;
                    }
                }
            }
        }
        push = p_push; pop = p_pop;
    }
    pop_t pop_ = nullptr;
    RoctxRange(const Handle *h, const char *name);
    ~RoctxRange() { if (pop_) pop_(); }
};
inline RoctxRange::RoctxRange(const Handle *h, const char *name)
{
    if (!h || h->opt[SWE2D_OPT_ROCTX] <= 0) return;
    push_t push;
    resolve(push, pop_);
    if (push) push(name); else pop_ = nullptr;
}


inline bool has_sources(const Handle *h)
{
    for (int i = 0; i < SWE2D_FIELD_COUNT; i++) if (h->field[i]) return true;
    if (h->n_cfarms > 0) return true;                  // (discrete farms are a pass of their own after the stage kernel)
    return h->scalar[SWE2D_SCALAR_LINEAR_DRAG] >= 0 || h->scalar[SWE2D_SCALAR_QUADRATIC_DRAG] >= 0
           || h->scalar[SWE2D_SCALAR_MANNING_DRAG] >= 0 || h->scalar[SWE2D_SCALAR_NIKURADSE] >= 0;
}

inline int grid_for(int n) { return (n + 255)/256; }

// a forcing the device evaluates in front of every stage launch, by the handle's clock: a tide table, an atmospheric record
inline bool forced(const Handle *h) { return h->tide.n > 0 || h->atm.n_t > 0; }

// options (swe2d_set_option): on unless switched off / the value in seconds with its default
inline bool opt_on(const Handle *h, int o) { return h->opt[o] != 0; }
inline double opt_seconds(const Handle *h, int o, double dflt) { return h->opt[o] > 0 ? 1e-3*h->opt[o] : dflt; }

// ---- stage launches (swe2d_api.hip)
// Where the 16-B connectivity records (swe2d_conn.h) pay: launches that stream from memory - from ~250 k cells, where the 8 B
// they save per cell are 2-3 % of a stage's traffic (profiles/r05zc: 1 M triangles 113.1 -> 110.3 us per step, 500 k 63.6 -> 62.7);
// a launch of 125 k cells is latency-bound and the ~20 integer instructions of the decode make it 1 % slower (24.0 against 23.8),
// and so are the kernels bound by their arithmetic (wetting-drying + Manning: 80.5 against 79.8; tracer with fused diffusion).
inline bool conn_pays(const Handle *h, int n_cells_of_launch, bool arithmetic_bound)
{
    const int o = h->opt[SWE2D_OPT_COMPACT_IDX];
    return h->idxc && o != 0 && (o == 2 || (n_cells_of_launch >= 250000 && !arithmetic_bound));
}
inline TileSet &pair_tiles(Handle *h) { return h->npc == 4 ? h->fuseq : h->fuse; }     // the stage pair's tables for the handle's cell type
int fuse12_build(Handle *h);
int launch_fuse12(Handle *h, int cell_end);
int fuse123_build(Handle *h);
int launch_fuse123(Handle *h, int cell_end);
int capture_parity_check(Handle *h);                    // SWE2D_ERR_UNSUPPORTED once after a capture that swapped the state buffers an odd number of times
bool stream_capturing(Handle *h, unsigned long long *id = nullptr);   // is the handle's stream capturing (and which capture)?
void stage_written(Handle *h, bool s0, bool s1);        // a launch left U(1) / U(2) in buffers B / C (none of it inside a capture)
inline void stage_invalidate(Handle *h) { h->stage_valid[0] = h->stage_valid[1] = false; }   // neither buffer holds a stage solution of the current state
inline void swap_state_buffers(Handle *h) { std::swap(h->state[0], h->state[1]); stage_invalidate(h); }   // A and B change places: B holds an older state, no stage solution
// ---- how a step is launched (swe2d_plan.hip)
enum StepPath : unsigned { kStages = 0, kPair = 1, kTriple = 2, kFlow = 4 };   // three stage launches | fused pair + stage 3 | three-stage kernel | dataflow kernel
// who asks: swe2d_advance on a whole mesh | a whole-mesh step without the dataflow kernel (swe2d_advance_coupled, swe2d_advance_timed per
// launch) | a partition's stage pair (swe2d_solve_stage_pair_cells) | a partition's whole step (swe2d_fused_step_info)
enum StepCaller { kAdvance, kWholeStep, kPartitionPair, kPartitionStep };
unsigned step_kernels(const Handle *h);                 // the kernels (StepPath bits) that cover the handle's configuration, whatever its size
StepPath step_plan(Handle *h, StepCaller who, StepPath at_most = kFlow);        // the path the caller takes by size and options
int step_ready(Handle *h, StepCaller who, StepPath at_most, StepPath *path);    // ... with its tile tables built, or the next path without
int whole_step_path(Handle *h, StepCaller who, StepPath *path);                 // ... of a whole-mesh step that may be inside a stream capture
inline int launches_per_step(StepPath p) { return p == kTriple ? 1 : (p == kPair ? 2 : 3); }
int step_launch(Handle *h, StepPath path, int i);       // launch i of a whole-mesh step by kStages / kPair / kTriple
int step_swe(Handle *h, StepCaller who, int n_steps);   // n_steps SSPRK33 steps of the shallow-water state on the whole mesh (kAdvance / kWholeStep)
bool fuse12_tiles_pay(const Handle *h, int n_tiles);    // are the stage pair's tiles worth it (else fuse_state = -1)?
bool flow_fits(Handle *h);                              // every 64-cell block of the handle resident at once
void fill_stage_args(Handle *h, SweStageArgs &a, int in, int u0, int out, double a0, double a1, double beta, int c0, int c1);
int launch_stage(Handle *h, int in, int u0, int out, double a0, double a1, double beta, int c0, int c1);
int stage_on_range(Handle *h, int i_stage, int c0, int c1);
// per-facet values -> the facet planes of a boundary field; a per-vertex coefficient -> the device (swe2d_api.hip)
int scatter_facet_values(Handle *h, double *planes, int n, const int32_t *cells, const int32_t *facets,
                         const double *values, int ncomp, int nval);
int upload_vertex_coefficient(Handle *h, const double *vertex_values, DevArray<double> &dev);
// ---- dataflow stage loop (swe2d_api_flow.hip)
int flow_build(Handle *h, const int32_t *order);
int flow_capacity(Handle *h);
int flow_build_exchange(Handle *h);
int launch_flow(Handle *h, int n_stages, const int32_t *cell_end, int n_cycles = 0);
int flow_check(Handle *h);
// ---- peer-to-peer halo (swe2d_api_p2p.hip)
size_t p2p_channel_offset(const int *width, int c, int n_recv);
void p2p_close(Handle *h);                              // closes the peers' mappings, frees the landing zone (swe2d_destroy)
// ---- tidal turbine farms (swe2d_turbine.hip)
bool farm_capturing(Handle *h);
int farm_upload_table(Handle *h);                       // the device's copy of the farms' constants, after every change of a slot
int farm_rows_alloc(Handle *h, int capacity);
// ---- discrete turbine farms (swe2d_dfarm.hip)
int dfarm_launch_drag(Handle *h, int in, int out, double beta, int c0, int c1);   // after a stage launch: U_out[uv] += beta*dt*M^-1 R_farm(U_in)
int dfarm_launch_power(Handle *h, unsigned long long *row);                       // the discrete farms' power of buffer A into their slots of `row`
// ---- harmonic tidal boundary elevation (swe2d_tide.hip)
int tide_launch(Handle *h, double t);                   // one launch: the boundary elevation at time t into the elevation planes of bc_field
double tide_stage_time(const Handle *h, int step, int i_stage);   // time of a stage of step `step` of the advance being enqueued (i_stage < 0: ForwardEuler)
int forcing_refuse_capture(Handle *h);                  // SWE2D_ERR_UNSUPPORTED where a handle with a tide table or an atmospheric record is stepped inside a stream capture
// ---- atmospheric forcing (swe2d_atm.hip)
int atm_launch(Handle *h, double t);                    // one launch: wind stress and pressure at time t into their field planes
int atm_check_advance(Handle *h, int n_steps, bool forward_euler);   // SWE2D_ERR_INVALID_ARGUMENT where a stage time of the advance leaves the record
// ---- reacting tracers (swe2d_reaction.hip)
int reaction_launch(Handle *h, int id, int in, int c0, int c1);   // in front of a stage launch of tracer `id` reading buffer `in`: its source planes on [c0, c1)
// ---- suspended sediment + Exner (swe2d_sediment.hip)
int sediment_source_launch(Handle *h, int in, int c0, int c1);   // in front of a stage launch of the sediment tracer reading buffer `in`
int sediment_update_launch(Handle *h);                  // E, D, equilibrium from buffer A + the 'equilibrium' facets of the value table
int exner_launch(Handle *h);                            // one bed update from the sediment tracer's buffer A and / or the bedload planes
int bedload_update_launch(Handle *h);                   // q_b and its contribution planes from buffer A and the current bed
int slide_update_launch(Handle *h);                     // alpha, beta and the slide's contribution planes from the current bed
bool bedload_fused(const Handle *h);                    // sediment_update_launch writes them too (one launch for both closures)
inline bool exner_steps(const Handle *h)                // the bed moves after every step of swe2d_advance_coupled / swe2d_advance
{
    return (h->sed.on && h->sed.par.solve_exner) || (h->bed.on && h->bed.par.solve_exner) || (h->slide.on && h->slide.par.solve_exner);
}
// ---- Smagorinsky eddy viscosity (swe2d_smag.hip)
int smag_update_launch(Handle *h);                      // in front of a step: nu_v from buffer A (cell pass + vertex pass)

}  // namespace swe2d_impl
using namespace swe2d_impl;
