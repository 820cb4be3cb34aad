/*
 * swe2d.h - C ABI of the MI355X-native explicit 2D shallow-water stepper (libswe2d_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of thetisproject/thetis: the SSPRK33 time step of the
 * DG-P1 ('dg-dg', degree 1) 2D shallow water equations.  In the reference that path is
 *
 *   FlowSolver2d.iterate()                         thetis/solver2d.py:974-1144
 *     -> timestepper.advance(t, update_forcings)   thetis/rungekutta.py:949-952   (ERKGenericShuOsher)
 *        -> solve_stage(i): LinearVariationalSolver.solve() of  M k = dt R(U)     thetis/rungekutta.py:930-946
 *           R = ShallowWaterEquations.residual('all', U, U, ...)                  thetis/shallowwater_eq.py:922-928
 *
 * and the only contract FlowSolver2d has with a stepper is TimeIntegratorBase (thetis/timeintegrator.py:13-39):
 * ctor(equation, solution, fields, dt, options, bnd_conditions), initialize(solution), advance(t, update_forcings),
 * set_dt(dt); state is exchanged in place through `solution`.  Every entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no exceptions cross the boundary: every function
 * returns 0 on success or a negative swe2d_status, and swe2d_last_error() gives the message.
 *
 * Host arrays use the reference's (Firedrake-side, [FD-assumed]) dof layout: cell c owns DG nodes 3c..3c+2 (= its
 * vertices in cell_vertices order); uv is (3N,2) row-major, eta is (3N).  Device layout is private (SoA planes).
 *
 * Threading: one host thread drives a handle; functions are not re-entrant per handle.  All work is enqueued on
 * the handle's HIP stream; functions that return data to host pointers synchronise that stream.
 */
#ifndef SWE2D_H
#define SWE2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWE2D_ABI_VERSION 12
#define SWE2D_MAX_MARKERS 16          /* boundary markers must be in 1..SWE2D_MAX_MARKERS-1 */

typedef enum {
    SWE2D_OK = 0,
    SWE2D_ERR_INVALID_ARGUMENT = -1,
    SWE2D_ERR_NO_DEVICE = -2,          /* no HIP device / HIP runtime error at init: the library never falls back to the CPU */
    SWE2D_ERR_HIP = -3,
    SWE2D_ERR_UNSUPPORTED = -4,
    SWE2D_ERR_NOT_FINITE = -5
} swe2d_status;

/* Boundary-condition kinds, bitmask.  Keys of bnd_functions['shallow_water'][marker]
 * (thetis/shallowwater_eq.py:232-296).  0 = closed (land) boundary. */
#define SWE2D_BC_ELEV 1
#define SWE2D_BC_UV   2
#define SWE2D_BC_UN   4
#define SWE2D_BC_FLUX 8
/* Function-valued boundary data (e.g. a tidal elevation field on an open boundary, updated by update_forcings): OR the
 * flag into `kind`; the value is then read from the nodal field given to swe2d_set_bc_field instead of values[]. */
#define SWE2D_BC_ELEV_FIELD 16
#define SWE2D_BC_UV_FIELD   32
#define SWE2D_BC_UN_FIELD   64
#define SWE2D_BC_FLUX_FIELD 128

/* Nodal coefficient fields, `fields` dict of get_swe_timestepper (thetis/solver2d.py:547-559). */
typedef enum {
    SWE2D_FIELD_CORIOLIS = 0,              /* options.coriolis_frequency      shallowwater_eq.py:623-634 */
    SWE2D_FIELD_ATMOSPHERIC_PRESSURE = 1,  /* options.atmospheric_pressure    shallowwater_eq.py:658-663 */
    SWE2D_FIELD_MOMENTUM_SOURCE = 2,       /* options.momentum_source_2d (3N,2) shallowwater_eq.py:805-811 */
    SWE2D_FIELD_VOLUME_SOURCE = 3,         /* options.volume_source_2d        shallowwater_eq.py:825-831 */
    SWE2D_FIELD_WIND_STRESS = 4,           /* options.wind_stress (3N,2)      shallowwater_eq.py:643-649 */
    /* spatially varying drag coefficients (nodal DG values); a field replaces the scalar of the same name, the same
     * exclusions apply (at most one of quadratic / Manning / Nikuradse, shallowwater_eq.py:686-696) */
    SWE2D_FIELD_LINEAR_DRAG = 5,           /* options.linear_drag_coefficient as a Function */
    SWE2D_FIELD_QUADRATIC_DRAG = 6,        /* options.quadratic_drag_coefficient as a Function */
    SWE2D_FIELD_MANNING_DRAG = 7,          /* options.manning_drag_coefficient as a Function */
    SWE2D_FIELD_NIKURADSE = 8,             /* options.nikuradse_bed_roughness as a Function */
    SWE2D_FIELD_COUNT = 9
} swe2d_field;

/* Scalar coefficients (Constants in the reference). */
typedef enum {
    SWE2D_SCALAR_LINEAR_DRAG = 0,          /* options.linear_drag_coefficient     shallowwater_eq.py:734-740 */
    SWE2D_SCALAR_QUADRATIC_DRAG = 1,       /* options.quadratic_drag_coefficient  shallowwater_eq.py:683,699-700 */
    SWE2D_SCALAR_MANNING_DRAG = 2,         /* options.manning_drag_coefficient    shallowwater_eq.py:685-688 */
    SWE2D_SCALAR_NORM_SMOOTHER = 3,        /* options.norm_smoother               shallowwater_eq.py:700 */
    SWE2D_SCALAR_NIKURADSE = 4,            /* options.nikuradse_bed_roughness     shallowwater_eq.py:692-700 (kappa = 0.4) */
    SWE2D_SCALAR_COUNT = 5
} swe2d_scalar;

/* Library options: how the path is carried out, never what it computes (every setting gives the same bits; the parity tests
 * force each in turn).  Read by the library from the handle only - it never looks at the process environment; the THETIS_AMD_*
 * variables of the same names are a convenience of the Python binding (thetis_amd/_lib.py: OPTION_ENV), applied once after
 * swe2d_create.  value -1 = the library's own rule.  No reference counterpart (Firedrake's analogue is the
 * solver_parameters / PyOP2 configuration a script may pass, thetis/options.py:145-152). */
typedef enum {
    SWE2D_OPT_FUSED_STAGES = 0,   /* stages of a step in one launch by overlapped tiles (csrc/swe2d_fuse.h): -1 from 250 k triangles
                                     when the numbering gives compact tiles - and all three stages in one launch on whole meshes
                                     without source terms (swe2d_fused_triple_info): from 131 073 cells where the caller handed in
                                     patches (swe2d_fused_set_triple_tiles), from 2.5 M otherwise; 0 never; 1 the pair on every mesh the
                                     kernel covers; 2 the pair by the size rule, never the triple; 3 the triple on every whole mesh */
    SWE2D_OPT_FLOW = 1,           /* swe2d_advance takes the dataflow stage loop (csrc/swe2d_flow.h) where it applies: -1 / 1 yes, 0 no */
    SWE2D_OPT_FLOW_WD = 2,        /* ... also with wetting-drying: -1 / 1 yes, 0 no */
    SWE2D_OPT_BND_INLINE = 3,     /* triangle stage kernels: boundary facets from registers (1) or by the epilogue that reloads them (0);
                                     -1: inline, with wetting-drying the epilogue.  0 also keeps the fused / dataflow kernels away */
    SWE2D_OPT_LDSX = 4,           /* in-wave neighbour traces through LDS: -1 in launches beyond the Infinity Cache, 0 / 1 forced */
    SWE2D_OPT_ALTERNATE = 5,      /* alternating launch direction: -1 in launches beyond the Infinity Cache, 0 / 1 forced */
    SWE2D_OPT_COMPACT_IDX = 6,    /* 16-B connectivity records: -1 / 1 in launches of >= 250 k cells, 0 never, 2 in every launch */
    SWE2D_OPT_VISC_FUSION = 7,    /* triangles: viscosity inside the stage kernel (-1 / 1) or as a separate pass (0) */
    SWE2D_OPT_WALL_FAST = 8,      /* closed walls on a path of their own in the boundary code (-1 / 1) or through the general one (0) */
    SWE2D_OPT_FLOW_POLL = 9,      /* granule loads per polling trip of the dataflow kernel: -1 by the blocks' rim facets, else 3 ... 9 */
    SWE2D_OPT_FLOW_CAPACITY = 10, /* resident 64-cell blocks the dataflow kernel may assume: -1 what the device holds (tests force less) */
    SWE2D_OPT_FLOW_TIMEOUT_MS = 11, /* bound of every wait inside the dataflow kernel, default 2000 */
    SWE2D_OPT_P2P_TIMEOUT_MS = 12,  /* bound of the peer-to-peer waits, default 5000 */
    SWE2D_OPT_P2P_ZONE = 13,      /* landing zone memory: -1 first that works, 1 uncached, 2 fine-grained, 3 ordinary device memory */
    SWE2D_OPT_ROCTX = 14,         /* 1: ROCTx ranges around the entry points that advance the state (rocprofv3 --marker-trace) */
    SWE2D_OPT_COUNT = 15
} swe2d_option;

/* Mesh = what FlowSolver2d(mesh2d, bathymetry_2d) receives (thetis/solver2d.py:81-147) flattened to arrays.
 * Triangles (nodes_per_cell == 3, DG-P1) or convex quadrilaterals (nodes_per_cell == 4, DQ-1), counter-clockwise.  A mesh of
 * parallelograms (every quadrilateral mesh the reference builds itself) takes the kernels with a constant Jacobian and the tensor
 * mass inverse; one cell that is not a parallelogram selects the general bilinear kernels for the whole mesh (Jacobian per
 * quadrature point, 4 x 4 mass solve per cell, mass-weighted cell means; thetis/solver2d.py:340-345 accepts any quadrilateral
 * mesh) - every option of the path runs on either kind.
 * Local facet f joins local vertices f and (f+1)%nodes_per_cell; all [..][3] shapes below read [..][nodes_per_cell].
 * In a multi-GPU partition the first n_owned cells are updated by this handle and cells n_owned..n_cells-1 are
 * ghost cells (one layer, facet-adjacent) whose state arrives through swe2d_halo_*. */
typedef struct {
    int32_t n_cells;
    int32_t n_owned;                   /* == n_cells on a single device */
    int32_t n_vertices;
    int32_t nodes_per_cell;            /* 3 or 4 */
    const int32_t *cell_vertices;      /* [n_cells][3] */
    const double  *vertex_xy;          /* [n_vertices][2] */
    const int32_t *cell_neighbours;    /* [n_cells][3]  >=0: neighbour cell, <0: -(boundary marker) */
    const int8_t  *cell_neighbour_facets; /* [n_cells][3] local facet id of the shared facet inside the neighbour */
    const double  *bathymetry;         /* [n_vertices] CG-P1 bathymetry, positive down (fields.bathymetry_2d) */
    const double  *boundary_len;       /* [SWE2D_MAX_MARKERS] total length per marker (utility.py:821-832), may be NULL on
                                          a single device (computed); REQUIRED for partitions (global lengths) */
} swe2d_mesh;

/* The ModelOptions2d entries the path reads (thetis/options.py:583-733). */
typedef struct {
    double  g_grav;                              /* physical_constants['g_grav'] = 9.81 */
    double  dt;                                  /* options.timestep */
    int32_t use_nonlinear_equations;             /* default 1 */
    int32_t use_lax_friedrichs_velocity;         /* default 1 */
    double  lax_friedrichs_velocity_scaling_factor; /* default 1.0 */
    int32_t device_id;                           /* HIP device ordinal */
} swe2d_params;

typedef struct swe2d_handle swe2d_handle;

/* version / capability */
int  swe2d_abi_version(void);
/* How the triangle kernels read the connectivity: out[0] = 1 when from the 16-B records (neighbour and vertex ids as differences
 * to the cell's own, csrc/swe2d_kernels.h swe_conn_pack; in launches of >= 250 k cells, where it pays;
 * SWE2D_OPT_COMPACT_IDX = 0 keeps the 24-B records everywhere, = 2 takes the 16-B records in every launch), out[1] = the number
 * of cells whose differences did not fit and which read the 24-B record after all.  Results do not depend on it. */
int  swe2d_connectivity_info(swe2d_handle *h, int32_t out[2]);
/* Stages 1 and 2 of a step in ONE launch by overlapped tiles (csrc/swe2d_fuse.h: 192 interior cells + their ring per workgroup,
 * the first stage's result never leaves the chip), stage 3 as a stage launch: what swe2d_advance and swe2d_advance_coupled do from
 * 250 k triangles without wetting-drying or viscosity (source terms are covered), when the cell numbering gives compact tiles, and
 * what swe2d_solve_stage_pair_cells does on a partition of that size (SWE2D_OPT_FUSED_STAGES = 0:
 * never, = 1: on every such mesh).  Same results bit for bit; the intermediate stage_sol[0] = U(1) then never reaches the state buffers
 * (swe2d_get_stage_state(h, 0) after such a step returns SWE2D_ERR_UNSUPPORTED, not a stale buffer).
 * out[0] = 1 when swe2d_advance would take it now (builds the tile tables on first use), out[1] = tiles, out[2] = ring cells
 * (cells evaluated redundantly in stage 1), out[3] = cells. */
int  swe2d_fused_pair_info(swe2d_handle *h, int32_t out[4]);
/* The tiles are cut from consecutive cells of an ORDER (default: the numbering of swe2d_mesh, NULL restores it): a partition whose
 * ghost layers are appended to its numbering layer by layer passes one in which every ghost cell sits next to the owned cells it
 * touches (cf. swe2d_flow_set_order).  Results do not depend on it.  Drops tile tables built before; synchronises the stream. */
int  swe2d_fused_set_order(swe2d_handle *h, const int32_t *cells_in_tile_order);
/* ALL three stages of a step in one launch (by itself from 2.5 M triangles, from 131 073 with the caller's patches - see SWE2D_OPT_FUSED_STAGES; = 3 forces it; csrc/swe2d_fuse.h swe_fuse123_kernel: tiles of interior +
 * two rings, U(1) and U(2) stay on chip, U(3) goes to the second state buffer and the two change places - so not inside a stream
 * capture, where swe2d_advance keeps the fused pair): whole meshes; out[0] = 1 when swe2d_advance would take it now (builds
 * the tile tables), out[1] = tiles, out[2] / out[3] = cells of the first / second rings (stage 1 is evaluated on interior + both,
 * stage 2 on interior + the first).  Same results bit for bit. */
int  swe2d_fused_triple_info(swe2d_handle *h, int32_t out[4]);
/* The two-ring tiles alone may be cut from an order of their own, with positions at which a tile must begin (tile_starts, n_starts
 * of them; NULL / 0: none): compact patches sized for interior + two rings (thetis_amd/ordering.py triple_tile_order: 11 x 8 quads of
 * a RectangleMesh) instead of as many consecutive cells as fit.  cells_in_tile_order = NULL: the order of swe2d_fused_set_order.
 * Results do not depend on it.  Replaces nothing in the reference (Firedrake's PyOP2 has no tiling to steer). */
int  swe2d_fused_set_triple_tiles(swe2d_handle *h, const int32_t *cells_in_tile_order, const int32_t *tile_starts, int32_t n_starts);
/* A PARTITION's whole step in one launch (round 6, last): stage 3 on cells [0, cell_end), the last of the step's three shrinking ranges
 * (thetis_amd/partition.py stage_range); stages 1 and 2 are evaluated on the tiles' supersets of theirs and never leave the chip.  The
 * result goes to the second state buffer and the two change places: inside a stream capture call it an EVEN number of times per
 * captured sequence (the pointers a replay uses are those of the capture).  The count is kept per capture: a capture with an odd
 * number is reported as SWE2D_ERR_UNSUPPORTED, once, by the next call outside a capture that reads or writes the state (that call does
 * nothing else), and its host-side swap is undone - the state is then the one from before the capture, which ran nothing.  Build the
 * tables before (swe2d_fused_step_info): inside a capture swe2d_fused_step_info / swe2d_fused_triple_info allocate nothing and answer
 * out[0] = 0 while the tables are not built.
 * Cells of the state beyond cell_end hold stale values afterwards (ghost cells the next exchange rewrites).  SWE2D_ERR_UNSUPPORTED
 * where the kernel does not cover the handle (quadrilaterals, wetting-drying, viscosity, source terms unless forced).
 * swe2d_fused_step_info: out[0] = 1 when the caller should take it (patches handed in with swe2d_fused_set_triple_tiles and more
 * cells than the dataflow kernel holds, or SWE2D_OPT_FUSED_STAGES = 3), out[1..3] as swe2d_fused_triple_info.  Same bits as
 * swe2d_solve_stage_cells x 3.  Replaces: one ERKGenericShuOsher.advance on a rank's cells (thetis/rungekutta.py:949-952). */
int  swe2d_solve_step_cells(swe2d_handle *h, int32_t cell_end);
int  swe2d_fused_step_info(swe2d_handle *h, int32_t out[4]);
int  swe2d_device_count(void);                                   /* number of visible HIP devices, <0 on error */

/* Shu-Osher coefficients the stage kernels use (host-only, needs no device): stage i computes
 * U_{i+1} = beta[i]*k_i + alpha0[i]*U_0 + alpha_in[i]*U_i  (alpha_in[0] multiplies U_0 itself).  Values are the output of
 * butcher_to_shuosher_form (thetis/rungekutta.py:13-87) for SSPRK33Abstract (rungekutta.py:342-346). */
void swe2d_ssprk33_coefficients(double alpha0[3], double alpha_in[3], double beta[3]);

/* lifetime: replaces ERKGenericShuOsher.__init__/update_solver (rungekutta.py:877-924).
 * One handle = one device.  The kernels address a group of nodes_per_cell SoA planes through one 4 GiB buffer resource with
 * 32-bit offsets: nodes_per_cell * n_cells * 8 bytes must stay below 2^32 (about 178 M triangles / 134 M quadrilaterals per
 * device), larger meshes return SWE2D_ERR_UNSUPPORTED and have to be partitioned (one handle per part). */
int  swe2d_create(const swe2d_mesh *mesh, const swe2d_params *params, swe2d_handle **out);
/* Partitions of ONE quadrilateral mesh must all take the same kernel family: the parallelogram kernels and the general bilinear
 * ones differ in the last bits on the same parallelogram cell, and a ghost cell must repeat its owner's arithmetic.  A handle
 * whose own cells are all parallelograms while the global mesh has a general cell is told so here (on = 1: general kernels;
 * on = 0: back to what the handle's own cells allow).  Call before the first step. */
int  swe2d_set_general_quadrilaterals(swe2d_handle *h, int on);
void swe2d_destroy(swe2d_handle *h);
const char *swe2d_last_error(const swe2d_handle *h);             /* h may be NULL: error of the last failed create */
/* library options (swe2d_option above); takes effect from the next call on */
int  swe2d_set_option(swe2d_handle *h, int option, int value);
int  swe2d_get_option(swe2d_handle *h, int option, int *value);

/* state: the mixed Function solution_2d = (uv_2d, elev_2d) (solver2d.py:410-413); host pointers */
int  swe2d_set_state(swe2d_handle *h, const double *uv, const double *eta);
int  swe2d_get_state(swe2d_handle *h, double *uv, double *eta);
/* the stage solution the reference assigns to `solution` after solve_stage(i_stage) (rungekutta.py:930-946): i_stage 0, 1 read
 * the buffers holding U1, U2; i_stage 2 (= swe2d_get_state) the step result.  The reference's stage_sol[i] always is what stage i
 * left; here the fused stage pair keeps U1, the dataflow kernel U1 and U2, on chip: when the step made last did not leave the asked
 * stage solution in memory (or no stage has run since swe2d_set_state / a restore, or the step made last was a ForwardEuler step,
 * or a swap of the state buffers) the call returns SWE2D_ERR_UNSUPPORTED - drive the step with swe2d_solve_stage to read
 * intermediate stages.  Stage launches made inside a stream capture execute nothing when they are recorded and the host never sees
 * their replays: after any state-writing launch recorded in a capture, i_stage 0 and 1 are refused (before and after a replay) until
 * the next eager step writes them again.  i_stage 2 reads buffer A, which a replay writes in place. */
int  swe2d_get_stage_state(swe2d_handle *h, int i_stage, double *uv, double *eta);
/* Save (restore = 0) / bring back (restore = 1) the time-stepping state - the step result and every tracer - in a device-side
 * copy, exactly, without the host: for steps that have to be undone (graph capture warm-ups, verification replays, benchmarks).
 * No reference counterpart (there `solution.assign(saved)` does it; here swe2d_get_state + swe2d_set_state is exact only without
 * wetting-drying: with it the device carries the displaced depth D = (H + sqrt(H^2 + alpha^2))/2 instead of eta, which it hands
 * out and takes in through the closed forms of thetis/utility.py:975-996 - the identity up to rounding, not bit for bit).
 * Enqueued on the handle's stream. */
int  swe2d_state_snapshot(swe2d_handle *h, int restore);         /* slot 0 */
/* ... in one of SWE2D_SNAPSHOT_SLOTS independent slots: a caller that keeps a long-lived copy (the start of a verification window)
 * and needs short-lived ones in between (graph capture warm-ups) gives each its own */
#define SWE2D_SNAPSHOT_SLOTS 2
int  swe2d_state_snapshot_slot(swe2d_handle *h, int slot, int restore);

/* TimeIntegrator.set_dt (timeintegrator.py:70-73) */
int  swe2d_set_dt(swe2d_handle *h, double dt);

/* bnd_functions['shallow_water'][marker] = {...} with constant values (shallowwater_eq.py:232-272).
 * kind = bitmask of SWE2D_BC_*; values = {elev, u, v, un, flux}.  May be called between stages
 * (update_forcings, rungekutta.py:933-934). */
int  swe2d_set_bc(swe2d_handle *h, int marker, int kind, const double values[5]);

/* Function-valued boundary data of ONE marker (bnd_functions[...][marker][key] = Function): nodal DG values of the whole
 * mesh in the host layout, which = 0: elevation (kN), 1: velocity (kN,2), 2: normal velocity (kN), 3: flux (kN).  Only the
 * nodes of boundary facets carrying `marker` are copied (stored per facet, so the two boundaries meeting at a corner cell
 * keep their own values).  Select the field with the SWE2D_BC_*_FIELD bit in swe2d_set_bc.  May be called between stages. */
int  swe2d_set_bc_field(swe2d_handle *h, int which, int marker, const double *nodal);
/* The same data as a COMPACT list - what update_forcings should cost per call (a tidal elevation Function re-evaluated at
 * t + c_i dt, rungekutta.py:933-934: a few KB instead of the whole nodal field): entry t is boundary facet facets[t] of cell
 * cells[t] (caller's cell numbering as passed to swe2d_create), values[t][j][c] the value at the facet's first (j = 0) and
 * second (j = 1) node, component c (2 components for which = 1, else 1).  Facets not listed keep their values. */
int  swe2d_set_bc_facets(swe2d_handle *h, int which, int32_t n_facets, const int32_t *cells, const int32_t *facets,
                         const double *values);

/* bnd_functions['shallow_water'][marker]['drag'] = C_D (BoundaryDragTerm, shallowwater_eq.py:704-725); negative: none */
int  swe2d_set_boundary_drag(swe2d_handle *h, int marker, double drag_coefficient);

/* coefficient fields: nodal DG-P1 values (3N) [(3N,2) for the momentum source and the wind stress] or NULL to switch the term off */
int  swe2d_set_field(swe2d_handle *h, int field, const double *nodal);
/* a CONTINUOUS P1 coefficient given per vertex (numbering of swe2d_mesh.vertex_xy), [n_vertices] or [n_vertices][2] for the
 * vector fields: the injection into the DG nodes happens on the device.  A time-dependent wind / pressure Function then costs
 * one value per vertex per update instead of one per DG node. */
int  swe2d_set_field_vertex(swe2d_handle *h, int field, const double *vertex_values);
/* scalar coefficients; a negative value switches the term off (norm_smoother: >= 0) */
int  swe2d_set_scalar(swe2d_handle *h, int which, double value);

/* options.use_wetting_and_drying + options.wetting_and_drying_alpha (thetis/options.py:872-884), alpha given at the mesh
 * vertices (constant or the P1 field of set_wetting_and_drying_alpha, solver2d.py:251-303).  The reference cannot run
 * SSPRK33 with wetting-drying; this enables the build's own explicit nodal formulation of the same
 * displaced depth: the continuity equation advances zeta = D - h, every stage ends with a positivity
 * limiter on the nodal depths (D >= 0.1 alpha) and a relaxation of the velocity on dry ground.  Enable it BEFORE
 * swe2d_set_state: the state is then brought to the admissible set (nodal depths through the limiter).  swe2d_diagnostics
 * reports int D dx, min D in slots 2, 3; swe2d_tendency returns the raw tendencies of (u, v, zeta). */
int  swe2d_set_wetting_and_drying(swe2d_handle *h, int enable, const double *alpha_vertex);

/* ERKGenericShuOsher.advance (rungekutta.py:949-952) repeated n_steps times, forcings constant in time.
 * Asynchronous: returns after enqueueing.
 * Buffer A: every step path leaves the step result in state buffer A (what swe2d_get_state reads and the next step starts from),
 * whatever the launches were.  The three-stage kernel writes U(3) into buffer B and swaps the host's pointers to A and B; inside a
 * stream capture swe2d_advance never takes it (a graph replays the pointers of its capture), so a captured swe2d_advance always ends
 * on the buffer it began on and can be replayed any number of times.  A capture that swapped an odd number of times
 * (swe2d_solve_step_cells) has its swap undone when it is reported, see swe2d_solve_step_cells. */
int  swe2d_advance(swe2d_handle *h, int n_steps);
/* ERKGenericShuOsher.solve_stage(i_stage) (rungekutta.py:930-946); i_stage = 0,1,2 in order. */
int  swe2d_solve_stage(swe2d_handle *h, int i_stage);
/* timeintegrator.ForwardEuler.advance (thetis/timeintegrator.py:115-165; 'ForwardEuler' in the steppers table,
 * solver2d.py:664) x n_steps:  U <- U + dt M^-1 R(U) - the first Shu-Osher stage followed by a buffer swap */
int  swe2d_advance_forward_euler(swe2d_handle *h, int n_steps);
/* n_steps steps bracketed by HIP events on the handle's stream; *ms_total = elapsed GPU time,
 * *ms_kernel_avg = mean duration of one stage kernel launch (events around every launch when per_launch != 0). */
int  swe2d_advance_timed(swe2d_handle *h, int n_steps, int per_launch, float *ms_total, float *ms_kernel_avg);
int  swe2d_synchronize(swe2d_handle *h);

/* parity hook: tendency k = M^-1 (dt R(U)) of the current state (what solver.solve() leaves in `tendency`,
 * rungekutta.py:940), host layout as the state. */
int  swe2d_tendency(swe2d_handle *h, double *k_uv, double *k_eta);

/* print_state norms + VolumeConservation2DCallback (solver2d.py:955-956, callback.py:350-364, utility.py:421-425):
 * out = { int eta^2 dx, int |u|^2 dx, int (eta+h) dx, min nodal (h+eta) } over the owned cells
 * (sums, not roots, so that partitions can be added). */
int  swe2d_diagnostics(swe2d_handle *h, double out[4]);
/* The same integrals as order-independent sums, for runs partitioned over several handles / ranks (the reference all-reduces its
 * diagnostics over the MPI ranks, thetis/callback.py:478-482; a floating-point all-reduce would make the printed norms and the
 * conservation checks depend on the partition in their last digits): every cell's contribution is split exactly into four
 * signed 38-bit limbs of units 2^40, 2^2, 2^-36, 2^-74, 2^-112, 2^-150 (what a term has below 2^-150 ~ 7e-46 is dropped) and the limbs are
 * summed as integers.  limbs[6 q + j] = limb j of
 * quantity q (int eta^2, int |u|^2, int (eta+h)); add the limbs of all partitions (int64, any order), then
 * swe2d_sum_limbs_to_double rounds a total to the nearest double.  swe2d_diagnostics returns exactly that for its own handle, so
 * one handle over the whole mesh and N handles over its partitions give identical doubles. */
int  swe2d_diagnostics_limbs(swe2d_handle *h, int64_t limbs[18], double *min_depth);
double swe2d_sum_limbs_to_double(const int64_t limbs[6]);

/* ---- SIPG horizontal viscosity: HorizontalViscosityTerm (thetis/shallowwater_eq.py:554-616), fields['viscosity_h'] =
 * options.horizontal_viscosity (solver2d.py:551).  nu is a constant (nu_vertex == NULL) or a continuous P1 field given per
 * vertex; sipg_factor = options.sipg_factor (options.py:730); the two flags are options.use_grad_div_viscosity_term and
 * use_grad_depth_viscosity_term (options.py:597-606).  Dirichlet boundary terms follow the velocity-type boundary
 * conditions set with swe2d_set_bc (:584-609).  With wetting and drying the depth of the grad-depth term is the displaced depth
 * and the dry-ground relaxation acts on the whole new velocity (viscous share included).  enable = 0 switches the
 * term off (viscosity_h None, :559-560). */
int  swe2d_set_viscosity(swe2d_handle *h, int enable, const double *nu_vertex, double nu_const, double sipg_factor,
                         int use_grad_div_viscosity_term, int use_grad_depth_viscosity_term);

/* ---- 2D tracers (thetis/tracer_eq_2d.py, non-conservative form) and the vertex-based P1DG limiter -----------------
 * A tracer is a scalar DG-P1 field (3N nodal values, same node layout as eta) advected by the CURRENT shallow-water
 * velocity of the handle.  Single-device handles only for now. */
int  swe2d_tracer_add(swe2d_handle *h, int *tracer_id);          /* options.add_tracer_2d (options.py:945-983) */
/* options.use_lax_friedrichs_tracer, lax_friedrichs_tracer_scaling_factor, tracer_advective_velocity_factor */
int  swe2d_tracer_set_options(swe2d_handle *h, int use_lax_friedrichs_tracer, double lax_friedrichs_tracer_scaling_factor,
                              double tracer_advective_velocity_factor);
int  swe2d_tracer_set_state(swe2d_handle *h, int tracer_id, const double *nodal);
int  swe2d_tracer_get_state(swe2d_handle *h, int tracer_id, double *nodal);
/* bnd_functions['tracer_2d'][marker] = {'value': c}; has_value = 0 restores the default boundary term
 * c (u.n) phi (tracer_eq_2d.py:177-191).  Velocity-type keys: swe2d_tracer_set_bc_velocity. */
int  swe2d_tracer_set_bc(swe2d_handle *h, int tracer_id, int marker, int has_value, double value);
/* external velocity of the tracer's boundary dict on `marker` (tracer_eq_2d.py:70-110): kind 0 = none (uv_ext = uv_in),
 * 1 = 'uv': (u, v), multiplied by tracer_advective_velocity_factor, 2 = 'un': normal velocity u (v unused),
 * 3 = 'flux': volume flux u out of the domain, uv_ext = factor * u / (H(elev_in) * boundary_len) n,
 * 4 = 'flux' with a constant 'elev' in the dict: the same with H(v) */
int  swe2d_tracer_set_bc_velocity(swe2d_handle *h, int tracer_id, int marker, int kind, double u, double v);
/* the same with Function-valued entries in compact form (tracer_eq_2d.py:100-109): values[n_facets][2] (kind 1 'uv':
 * [n_facets][2][2]) = the entry at the first and second node of boundary facet `facets[i]` of cell `cells[i]`; elev: the
 * constant 'elev' of a 'flux' entry (kind 4), ignored otherwise */
int  swe2d_tracer_set_bc_velocity_facets(swe2d_handle *h, int tracer_id, int marker, int kind, double elev, int32_t n_facets,
                                         const int32_t *cells, const int32_t *facets, const double *values);
/* Function-valued 'value' on `marker`: nodal DG values of the whole mesh in the host layout (kN); only cells with a
 * boundary facet carrying `marker` are copied (all their nodes: the diffusive boundary term uses the cell gradient) */
int  swe2d_tracer_set_bc_field(swe2d_handle *h, int tracer_id, int marker, const double *nodal);
/* compact form: values[t][i] = external value at node i of cell cells[t], stored for its boundary facet facets[t] */
int  swe2d_tracer_set_bc_facets(swe2d_handle *h, int tracer_id, int32_t n_facets, const int32_t *cells, const int32_t *facets,
                                const double *values);     /* then select them: swe2d_tracer_set_bc(..., has_value = 2, 0) */
int  swe2d_tracer_set_source(swe2d_handle *h, int tracer_id, const double *nodal);   /* SourceTerm tracer_eq_2d.py:281-298 */
/* options.tracer[label].use_conservative_form (options.py:543): the tracer field is the depth-integrated q = H*T and the
 * stage kernels evaluate ConservativeHorizontalAdvectionTerm / ConservativeSourceTerm (tracer_eq_2d.py:325-437) */
int  swe2d_tracer_set_conservative(swe2d_handle *h, int tracer_id, int use_conservative_form);
/* SIPG horizontal diffusion: HorizontalDiffusionTerm (tracer_eq_2d.py:226-278), fields['diffusivity_h-<label>'] =
 * options.tracer[label].diffusivity (solver2d.py:588); constant or per-vertex P1; sipg_factor_tracer options.py:732 */
int  swe2d_tracer_set_diffusivity(swe2d_handle *h, int tracer_id, int enable, const double *mu_vertex, double mu_const,
                                  double sipg_factor_tracer);
/* boundary term of the diffusion operator on `marker` (tracer_eq_2d.py:264-277): kind 0 = none (no boundary dict),
 * 1 = prescribed 'diff_flux' (-phi*diff_flux); otherwise -phi mu grad(c_up).n with c_up = s c + (1-s) c_ext, s the upwind
 * switch: 2 = constant 'value' (grad c_ext = 0), 3 = boundary dict without 'value' (c_ext = c), 4 = Function 'value' */
#define SWE2D_DIFF_BC_NONE 0
#define SWE2D_DIFF_BC_DIFF_FLUX 1
#define SWE2D_DIFF_BC_UPWIND 2
#define SWE2D_DIFF_BC_GRAD_IN 3
#define SWE2D_DIFF_BC_VALUE_FIELD 4
int  swe2d_tracer_set_diffusion_bc(swe2d_handle *h, int tracer_id, int marker, int kind, double diff_flux);
int  swe2d_tracer_solve_stage(swe2d_handle *h, int tracer_id, int i_stage);          /* rungekutta.py:930-946 for the tracer */
int  swe2d_tracer_tendency(swe2d_handle *h, int tracer_id, double *k_nodal);
int  swe2d_tracer_forward_euler(swe2d_handle *h, int tracer_id);                     /* one ForwardEuler step of the tracer */
/* partitions (one handle per GPU): the tracer stage on a local cell range, the limiter on cells [0, cell_end) with means
 * and vertex bounds taken over every local cell (the ghost layers must hold the neighbours' unlimited values), and the
 * tracer's part of the halo exchange (same cell lists as swe2d_halo_setup, nodes_per_cell doubles per cell) */
int  swe2d_tracer_solve_stage_cells(swe2d_handle *h, int tracer_id, int i_stage, int32_t cell_begin, int32_t cell_end);
/* ForwardEuler for a tracer on a partition: swe2d_tracer_solve_stage_cells(id, 0, begin, end) is the step from tracer buffer 0
 * into buffer 1 on a cell range; after the last range swe2d_tracer_swap_buffers makes buffer 1 the tracer (cf. swe2d_forward_euler_cells) */
int  swe2d_tracer_swap_buffers(swe2d_handle *h, int tracer_id);
int  swe2d_tracer_limit_cells(swe2d_handle *h, int tracer_id, int32_t cell_end);
int  swe2d_tracer_halo_pack(swe2d_handle *h, int tracer_id, int i_buffer, double *send_buf_dev);
int  swe2d_tracer_halo_unpack(swe2d_handle *h, int tracer_id, int i_buffer, const double *recv_buf_dev);         /* parity hook */
/* VertexBasedP1DGLimiter (thetis/limiter.py:48-198): topology of the mesh vertices (periodic meshes identify them);
 * optional - defaults to cell_vertices. */
int  swe2d_limiter_setup(swe2d_handle *h, int32_t n_topo_vertices, const int32_t *cell_topo_vertices);
int  swe2d_tracer_limit(swe2d_handle *h, int tracer_id);                             /* limiter.apply(field) */
/* out = { int T*H dx (comp_tracer_mass_2d, utility.py:437-445), int T dx, min nodal T, max nodal T } */
int  swe2d_tracer_diagnostics(swe2d_handle *h, int tracer_id, double out[4]);
/* limb sums (see swe2d_diagnostics_limbs) of { int T*H dx, int T dx } + { min, max } of the owned cells */
int  swe2d_tracer_diagnostics_limbs(swe2d_handle *h, int tracer_id, int64_t limbs[12], double minmax[2]);
/* GeneralCoupledTimeIntegrator2D.advance (coupled_timeintegrator_2d.py:93-113) x n_steps: SWE step (unless tracer_only),
 * then every tracer with the updated velocity, then the limiter (once per step).  Buffer A as for swe2d_advance: the shallow-water
 * step result ends in state buffer A (the tracer stages read the velocity from there) and every tracer's result in its buffer A. */
int  swe2d_advance_coupled(swe2d_handle *h, int n_steps, int tracer_only, int use_limiter);

/* profiling aid: n_times streaming copies of the 9 state planes (9*stride doubles read + written, 8 B per lane) to calibrate
 * the FETCH_SIZE / WRITE_SIZE counters on a known byte count; does not change the state */
int  swe2d_debug_calibration_copy(swe2d_handle *h, int n_times);
/* debugging aid: out[0] = bytes, out[1] = allocations of ordinary device memory the library holds right now, over all handles of
 * the process (a handle's landing zone of swe2d_p2p_create is not counted).  After the last swe2d_destroy both are what they were
 * before the first swe2d_create: a difference is a leak. */
int  swe2d_debug_live_device_memory(uint64_t out[2]);

/* ---- multi-GPU plumbing (one process per GPU; the exchange itself is done by the host with RCCL) ----
 * Replaces PyOP2's per-par_loop halo exchange [FD-assumed] by ONE exchange per time step: a partition carries three layers
 * of ghost cells (cells n_owned..n_cells-1, layer by layer); stage i is run on cells [0, n_owned + layers still needed),
 * see thetis_amd/partition.py.  send_cells: local ids of owned cells whose state peers need, grouped by peer;
 * recv_cells: local ids of the ghost cells in the order the peers' messages deliver them.  Buffers are device pointers
 * owned by the caller (cell-major: 3k doubles u0..u(k-1) v0.. e0.. per cell, [n][3k], k = nodes_per_cell, so per-peer
 * segments are contiguous).  i_buffer selects the state buffer (0 = the step result / stage-1 input).  On a handle without ghost
 * cells (n_owned = n_cells) recv_cells may name any cell: pack + unpack then copy between cells of the same mesh. */
int  swe2d_halo_setup(swe2d_handle *h, int32_t n_send, const int32_t *send_cells, int32_t n_recv, const int32_t *recv_cells);
int  swe2d_halo_pack(swe2d_handle *h, int i_buffer, double *send_buf_dev);
int  swe2d_halo_unpack(swe2d_handle *h, int i_buffer, const double *recv_buf_dev);
/* ---- peer-to-peer halo exchange through IPC-mapped device memory: the exchange as two kernels on the handle's stream (no host
 * or RCCL call in the step loop, capturable in a HIP graph).  Same role as swe2d_halo_pack + send/recv + swe2d_halo_unpack.
 * After swe2d_halo_setup:  swe2d_p2p_create (landing zone for n_recv cells x 2 slots per channel; channel 0 = the SWE state,
 * width 3k doubles per cell, channel 1 + t = tracer t, width k)  ->  swe2d_p2p_export (64-byte hipIpcMemHandle_t to hand to
 * the peers through any side channel, e.g. an all-gather; local_base serves peers inside the same process)  ->  every rank
 * swe2d_p2p_open()s the zones of the ranks it sends to  ->  swe2d_p2p_connect: peer i receives send-list cells
 * [send_offset[i], + send_count[i]) at cell offset remote_recv_offset[i] of ITS recv list (remote_n_recv[i] cells long) and
 * knows me as its sender number remote_flag_index[i]; n_from = number of ranks that send to me (their flag indices are
 * 0..n_from-1).  Then, per exchange and channel, on every rank in the same order: swe2d_p2p_push ... swe2d_p2p_wait_unpack.
 * A rank may run at most one exchange ahead of a peer (double-buffered slots); waits are bounded (SWE2D_OPT_P2P_TIMEOUT_MS,
 * default 5 s) and counted in swe2d_p2p_status.timeouts instead of hanging the device. */
#define SWE2D_IPC_HANDLE_BYTES 64
int  swe2d_p2p_create(swe2d_handle *h, int32_t n_channels, const int32_t *widths);
int  swe2d_p2p_export(swe2d_handle *h, void *ipc_handle_out, void **local_base, int32_t *zone_kind);
int  swe2d_p2p_open(swe2d_handle *h, const void *ipc_handle, void **remote_base);
int  swe2d_p2p_connect(swe2d_handle *h, int32_t n_peers, void *const *remote_base, const int32_t *send_offset,
                       const int32_t *send_count, const int32_t *remote_recv_offset, const int32_t *remote_flag_index,
                       const int32_t *remote_n_recv, int32_t n_from);
int  swe2d_p2p_push(swe2d_handle *h, int channel, int i_buffer);
int  swe2d_p2p_wait_unpack(swe2d_handle *h, int channel, int i_buffer);
/* the same for up to four channels (the shallow water state and the tracers at the end of a coupled exchange cycle) in ONE launch each
 * way: the channels' own kernels side by side, every channel with its own epochs and flags - interchangeable with the
 * single-channel calls, exchange by exchange */
int  swe2d_p2p_push_multi(swe2d_handle *h, int n, const int32_t *channels, const int32_t *i_buffers);
int  swe2d_p2p_wait_unpack_multi(swe2d_handle *h, int n, const int32_t *channels, const int32_t *i_buffers);
/* swe2d_p2p_push / swe2d_p2p_wait_unpack on a stream of their own (null: the handle's stream), so that the stage kernels of the
 * interior cells run while the halo travels - PyOP2 overlaps its halo exchange with the core of a par_loop the same way
 * [FD-assumed].  The caller orders the two streams with events; no synchronisation here. */
int  swe2d_set_exchange_stream(swe2d_handle *h, void *hip_stream);
int  swe2d_p2p_status(swe2d_handle *h, int64_t *epochs_sent, int64_t *epochs_received, int32_t *timeouts);
/* ERKGenericShuOsher.solve_stage restricted to cells [cell_begin, cell_end) (may include ghost layers) */
int  swe2d_solve_stage_cells(swe2d_handle *h, int i_stage, int32_t cell_begin, int32_t cell_end);
/* solve_stage(0) on [0, cell_end_0) followed by solve_stage(1) on [0, cell_end_1) (rungekutta.py:930-946; cell_end_1 <= cell_end_0
 * and every cell of the second range has its facet neighbours inside the first: the stage ranges of a partition's exchange cycle, or
 * the whole mesh twice) as ONE launch by overlapped tiles where that kernel covers the handle (swe2d_fused_pair_info), as the two
 * stage launches otherwise.  Either way state buffer 2 holds stage_sol[1] on [0, cell_end_1) afterwards, bit for bit the same;
 * stage_sol[0] is only left behind by the stage launches. */
int  swe2d_solve_stage_pair_cells(swe2d_handle *h, int32_t cell_end_0, int32_t cell_end_1);
/* ForwardEuler (timeintegrator.py:115-165) on a partition: the step from state buffer 0 into buffer 1 on a cell range;
 * after the last range of a step swe2d_swap_state_buffers makes buffer 1 the state (halo pack / unpack take the buffer
 * index).  Not capturable in a replayed graph across an odd number of swaps. */
int  swe2d_forward_euler_cells(swe2d_handle *h, int32_t cell_begin, int32_t cell_end);
int  swe2d_swap_state_buffers(swe2d_handle *h);
/* n_stages (a multiple of 3, at most 384) consecutive solve_stage calls - i.e. n_stages / 3 calls of ERKGenericShuOsher.advance
 * (rungekutta.py:949-952) - in ONE launch without a grid-wide barrier between the stages (csrc/swe2d_flow.h): stage s updates
 * the cells [0, cell_end[s]) (cell_end non-increasing, and every cell of stage s + 1's range has its facet neighbours inside
 * stage s's range: the shrinking ranges of a partition's exchange cycle, or n_owned throughout), a 64-cell block starts stage
 * s + 1 as soon as the trace values it needs from the blocks around it have arrived.  State buffer 0 (swe2d_get_state) ends bit for
 * bit as the swe2d_solve_stage_cells calls it stands for leave it; the intermediate stage solutions (swe2d_get_stage_state 0, 1)
 * are not produced.  swe2d_advance uses it on its own where it applies (SWE2D_OPT_FLOW = 0: never).  Needs every block of the
 * handle resident at once:
 * swe2d_flow_supported returns 0 when the mesh is too large for that (or the configuration is not covered: quadrilaterals,
 * viscosity; wetting-drying IS covered since round 5 - csrc/swe2d_k_flow_wd.hip, SWE2D_OPT_FLOW_WD = 0 leaves it to the stage
 * launches), 1 covered, 2 covered and without source terms;
 * SWE2D_ERR_UNSUPPORTED from swe2d_solve_flow otherwise.  Every wait inside the kernel is bounded (SWE2D_OPT_FLOW_TIMEOUT_MS, default 2 s); a timeout invalidates the
 * state and is reported as SWE2D_ERR_HIP by the next swe2d_synchronize / swe2d_get_state / swe2d_diagnostics
 * (swe2d_flow_status reads the count without failing). */
int  swe2d_solve_flow(swe2d_handle *h, int32_t n_stages, const int32_t *cell_end);
int  swe2d_flow_supported(swe2d_handle *h);
/* The same with the halo exchange of a partition INSIDE the launch, cell by cell: n_cycles exchange cycles (at most 64) of
 * stages_per_cycle stages each (at most 384 stages in all) on the ranges cell_end[0 .. stages_per_cycle) of ONE cycle.  Needs the
 * peer-to-peer halo connected with a LAST channel of width 18 (swe2d_p2p_create: nine 16-byte {value, push number} granules per
 * cell; the channel's epoch flags are not used).  Every cycle but the launch's first starts by receiving what the peers pushed at
 * the end of their previous cycle - every ghost cell's lane waits for the nine granules of ITS cell, so a ghost cell is ready as
 * soon as the one block of the peer that owns it has finished (the first cycle receives too if a push of an earlier launch is
 * still pending: pushes > receives of that channel in swe2d_p2p_status) - and ends by storing this rank's send cells as granules
 * into the peers' zones.  One launch replaces n_cycles x (swe2d_solve_flow + swe2d_p2p_push + swe2d_p2p_wait_unpack); the LAST
 * cycle's push is received by the next launch of this kind or by swe2d_flow_unpack_pending (needed before other kernels read the
 * ghost cells).  Cells sent to more than two peers are not supported (SWE2D_ERR_UNSUPPORTED).  Same results bit for bit. */
int  swe2d_solve_flow_exchange(swe2d_handle *h, int32_t n_cycles, int32_t stages_per_cycle, const int32_t *cell_end);
/* builds the tables of the former ahead of its first launch (which otherwise does it: allocations and a stream synchronisation,
 * not allowed inside a stream capture); after swe2d_halo_setup and swe2d_flow_set_order */
int  swe2d_flow_prepare_exchange(swe2d_handle *h);
int  swe2d_flow_unpack_pending(swe2d_handle *h);
/* The kernel's 64-cell blocks are consecutive cells of a FLOW ORDER (default: the numbering of swe2d_mesh).  A partition whose
 * ghost layers are appended to the numbering layer by layer (what the stage ranges need) passes an order - a permutation of
 * the cell ids - in which every ghost cell sits next to the cells it touches: blocks then stay compact patches and few facets
 * cross block rims.  Results do not depend on the order.  Synchronises the stream; not inside a stream capture. */
int  swe2d_flow_set_order(swe2d_handle *h, const int32_t *cells_in_flow_order);
int  swe2d_flow_status(swe2d_handle *h, int32_t *timeouts);
int  swe2d_debug_flow_poke(swe2d_handle *h, int32_t block, int32_t delta);      /* test hook: skews one block's stage counter */
/* test hook of the -DSWE_FLOW_DELAY build (an adversary for the granule protocol, csrc/swe2d_flow.h): one block sleeps at chosen
 * points of its stage loop; where = 1 before polling | 2 before publishing | 4 before an in-launch receive | 8 before an
 * in-launch push.  SWE2D_ERR_UNSUPPORTED in the product build. */
int  swe2d_debug_flow_delay(swe2d_handle *h, int32_t block, int32_t where, int32_t microseconds, int32_t every_nth_stage);
/* test hook of the -DSWE_FLOW_TEAR build (the adversary of the granules' check word, csrc/swe2d_flow.h): block `block` (-2: every
 * block, -1: off) makes the granule stores of every n-th publish in two halves, the half with the new tag first and the value
 * `microseconds` later; across_ranks: also the pushes into the peers' landing zones.  block = -3 asks whether the build's consumers
 * test the check word (1; 0 in the -DSWE_FLOW_NOCHECK negative control).  SWE2D_ERR_UNSUPPORTED in the product build. */
int  swe2d_debug_flow_tear(swe2d_handle *h, int32_t block, int32_t microseconds, int32_t every_nth_publish, int32_t across_ranks);
/* run on a caller-provided hipStream_t (e.g. torch's current stream) instead of the handle's own */
int  swe2d_set_stream(swe2d_handle *h, void *hip_stream);

/* ---- point probes: gauges / detectors (thetis/callback.py DetectorsCallback, Function.at) ------------------------------------
 * A probe set holds M points, each a device cell (the handle's own numbering, as every cell argument here) and its nodes_per_cell
 * nodal weights (barycentric on triangles, bilinear on quadrilaterals; the caller locates the points), and a list of fields:
 * SWE2D_PROBE_UV (2 components), SWE2D_PROBE_ELEV (1) or a tracer id >= 0 (1).  A row is, per point, the components of the fields
 * in list order: value = w0*v0 + w1*v1 + w2*v2 (+ w3*v3), left to right without contraction, v the nodal values of the state that
 * swe2d_get_state / swe2d_tracer_get_state would return (wetting-drying: eta, not the displaced depth) - the same bits as that sum
 * computed on the host from those arrays.  The rows are kept on the device (capacity rows); appending is one launch on the handle's
 * stream, no synchronisation, so a row may be appended after every step of a batch.  Every probe call inside a stream capture
 * returns SWE2D_ERR_UNSUPPORTED.  No reference counterpart at the C level (the reference interpolates onto a VertexOnlyMesh). */
#define SWE2D_PROBE_UV   (-1)
#define SWE2D_PROBE_ELEV (-2)
int  swe2d_probe_create(swe2d_handle *h, int32_t n_points, const int32_t *cells, const double *weights, int32_t n_fields,
                        const int32_t *fields, int32_t capacity, int32_t *probe_id);       /* weights: [n_points][nodes_per_cell] */
int  swe2d_probe_width(swe2d_handle *h, int32_t probe_id, int32_t *n_points, int32_t *n_components, int32_t *capacity);
/* one row of the current state (asynchronous); SWE2D_ERR_INVALID_ARGUMENT and nothing written when the set holds `capacity` rows */
int  swe2d_probe_append(swe2d_handle *h, int32_t probe_id);
/* the rows appended since the last read -> out [rows][n_points][n_components] (room for `capacity` rows), then the set is empty */
int  swe2d_probe_read(swe2d_handle *h, int32_t probe_id, double *out, int32_t *n_rows);
/* one row of the current state -> out [n_points][n_components], synchronously; the stored rows are not touched */
int  swe2d_probe_eval(swe2d_handle *h, int32_t probe_id, double *out);
int  swe2d_probe_destroy(swe2d_handle *h, int32_t probe_id);

/* ---- Tidal turbine farms (thetis/turbines.py:17-171, TurbineDragTerm shallowwater_eq.py:765-791).
 * A farm is a turbine type (constant or tabulated thrust), a nodal turbine density d(x) >= 0 that is zero outside the farm's
 * cells, and per-farm constants.  While a handle has farms, the momentum equation carries
 *     - c_t(|u|, H) d |u| u / H,   c_t = (C_T A_T + C_support A_support) / (2 alpha^2),
 *     alpha = upwind_correction ? (1 + sqrt(1 - (C_T A_T + C_support A_support)/(D_proj H)))/2 : 1,
 * integrated with the rule of the quadratic bottom drag, and every stepping path that does not evaluate it declines the handle:
 * the steps run as stage launches (swe2d_fused_pair_info / _triple_info / _step_info report 0, swe2d_flow_supported 0).
 * The thrust table: C_T = 0 below speeds[0], linear between entries, 0 from speeds[n_table - 1] on. */
#define SWE2D_MAX_FARMS 8
#define SWE2D_MAX_THRUST_TABLE 16
typedef struct {
    double  thrust_area_const;       /* C_T A_T of a constant-thrust turbine (n_table == 0) */
    double  support_area;            /* C_support A_support */
    double  rotor_area;              /* A_T = pi D^2 / 4 */
    double  projected_diameter;      /* D_proj (upwind correction) */
    double  power_const;             /* C_P of a constant-thrust turbine */
    double  rho0;                    /* physical_constants['rho0'] (power only) */
    int32_t upwind_correction;       /* 0 / 1 */
    int32_t n_table;                 /* 0: constant thrust; else 2 .. SWE2D_MAX_THRUST_TABLE entries, speeds strictly increasing */
    double  speeds[SWE2D_MAX_THRUST_TABLE];
    double  thrust[SWE2D_MAX_THRUST_TABLE];     /* C_T at speeds[] */
    double  power[SWE2D_MAX_THRUST_TABLE];      /* C_P at speeds[] */
} swe2d_turbine_params;
/* Sets (or replaces) farm `farm` in 0 .. SWE2D_MAX_FARMS-1.  density_nodal: [n_cells][nodes_per_cell], >= 0, zero in every cell
 * outside the farm; cells with a non-zero density form the farm's cell list (what the power kernel visits). */
int  swe2d_turbine_farm_set(swe2d_handle *h, int32_t farm, const swe2d_turbine_params *p, const double *density_nodal);
int  swe2d_turbine_farm_clear(swe2d_handle *h, int32_t farm);
/* Power of every farm slot (0 for an empty slot), int 0.5 rho0 A_T C_P(u3^(1/3)) u3 d dx with u3 = |u|^3 / alpha^3 and alpha formed
 * with the static bathymetry (TurbineFunctionalCallback, turbines.py:85-93, 233, 252), over the OWNED cells, of the state in buffer
 * A.  Synchronous.  _limbs: the same as order-independent limb sums [SWE2D_MAX_FARMS][6] (swe2d_diagnostics_limbs): partitions add
 * them as integers and round once with swe2d_sum_limbs_to_double - the doubles of one handle on the whole mesh. */
int  swe2d_turbine_power(swe2d_handle *h, double out[SWE2D_MAX_FARMS]);
int  swe2d_turbine_power_limbs(swe2d_handle *h, int64_t limbs[SWE2D_MAX_FARMS*6]);
/* Power rows on the device, as the probe rows: _reserve sets the capacity (and empties the store), _append enqueues ONE launch that
 * writes the limb sums of the current state into the next row (no synchronisation), _read synchronises, returns the rows appended
 * since the last read as doubles [n_rows][SWE2D_MAX_FARMS] and empties the store.  Refused inside a stream capture. */
int  swe2d_turbine_rows_reserve(swe2d_handle *h, int32_t capacity);
int  swe2d_turbine_rows_append(swe2d_handle *h);
int  swe2d_turbine_rows_read(swe2d_handle *h, double *out, int32_t *n_rows);

/* ---- Discrete tidal turbine farms (thetis/turbines.py:174-210): single turbines at coordinates, each a bump density
 *     d(x) = sum_t psi((x - x_t)/r) psi((y - y_t)/r) / (r^2 1.45661),   psi(s) = |s| < 1 ? exp(1 - 1/(1 - s^2)) : 0,   r = D_proj/2,
 * integrated with a rule of the caller's (n_q <= SWE2D_MAX_FARM_QUAD points; phi [n_q][nodes_per_cell] the basis functions at the
 * points in the node order of the state, w [n_q] weights that sum to 1 on the reference cell).  A discrete farm takes a slot of the
 * SWE2D_MAX_FARMS numbering and writes its power into the same rows as a continuous one, so swe2d_turbine_power, _power_limbs,
 * _rows_* and swe2d_turbine_farm_clear serve both kinds, and the fused and dataflow kernels decline the handle in the same way.
 * Its drag is not part of the stage kernels: after every stage launch one launch per discrete farm adds beta dt M^-1 R_farm(U_in)
 * to the velocity of the stage's output, over the farm's own cell list (a handle whose only farms are discrete runs the stage
 * kernel of a handle without farms).
 * _set: xy [n_turbines][2] (n_turbines >= 0; turbines outside the mesh are legal), cell_mask [n_cells] non-zero = the cell belongs
 * to the farm's subdomain.  The cell list - owned cells of the subdomain whose bounding box meets a turbine's square |x - x_t| < r,
 * |y - y_t| < r - is built on the host, the density is tabulated on the device at the rule's points of the listed cells, summed
 * over a cell's candidate turbines in the order of xy.  Not with wetting-drying (SWE2D_ERR_UNSUPPORTED); refused inside a stream
 * capture.  On an allocation failure (SWE2D_ERR_HIP) the slot keeps what it held.
 * _density_read: cells_out [n_list] the listed cells, density_out [n_q][n_list]; *n_list / *n_q are always set, the arrays may be
 * null to ask for the sizes.
 * _turbine_power: per turbine, int power * (the turbine's own bump) dx over the farm's cells, of the state in buffer A; each value
 * a limb sum rounded once.  Overlapping bumps split the farm's power: the values add up to the farm's entry of
 * swe2d_turbine_power up to rounding.  Synchronous. */
#define SWE2D_MAX_FARM_QUAD 64
int  swe2d_dfarm_set(swe2d_handle *h, int32_t farm, const swe2d_turbine_params *p, int32_t n_turbines, const double *xy,
                     const uint8_t *cell_mask, int32_t n_q, const double *phi, const double *w);
int  swe2d_dfarm_density_read(swe2d_handle *h, int32_t farm, int32_t *n_list, int32_t *n_q, int32_t *cells_out, double *density_out);
int  swe2d_dfarm_turbine_power(swe2d_handle *h, int32_t farm, double *out);

/* ---- Harmonic tidal elevation on open boundaries (thetis/forcing.py, TidalBoundaryForcing.set_tidal_field):
 *     eta_b(x, t) = mean(x) + sum_k amp_k(x) cos(omega_k t - phase_k(x))
 * evaluated on the device for the end nodes of the listed boundary facets, into the planes swe2d_set_bc_facets(h, 0, ...) writes
 * (markers take them with SWE2D_BC_ELEV_FIELD).  The argument and the running sum are formed left to right without contraction.
 * A handle with a tide table steps by stage launches with one tide launch in front of each, all enqueued by the one swe2d_advance /
 * swe2d_advance_forward_euler / swe2d_advance_coupled call; the fused kernels and the dataflow kernel decline it as they decline
 * turbine farms (the *_info calls and swe2d_flow_supported report 0; swe2d_solve_flow, swe2d_solve_step_cells and
 * swe2d_solve_stage_pair_cells return SWE2D_ERR_UNSUPPORTED).  The time is a kernel argument: inside a stream capture those advances
 * and every swe2d_tide_* call return SWE2D_ERR_UNSUPPORTED.  No reference counterpart at the C level. */
#define SWE2D_MAX_TIDE_CONSTITUENTS 32
/* Sets (or replaces) the table: n_facets (cell, facet) pairs in the caller's cell numbering as in swe2d_set_bc_facets, n_constituents
 * in 1 .. SWE2D_MAX_TIDE_CONSTITUENTS, omega[n_constituents], mean[n_facets][2], amp and phase [n_constituents][n_facets][2] (the two
 * end nodes of a facet: the cell's nodes facet and facet + 1).  Allocates the elevation planes if absent.  Keeps the clock. */
int  swe2d_tide_set(swe2d_handle *h, int32_t n_facets, const int32_t *cells, const int32_t *facets, int32_t n_constituents,
                    const double *omega, const double *mean, const double *amp, const double *phase);
int  swe2d_tide_clear(swe2d_handle *h);
/* The clock of the advances: step k of the next one starts at t_k = t_base + (double)(k_first + k)*dt - never an accumulated sum -,
 * its stage i is evaluated at t_k + c_i*dt, c = (0, 1, 1/2) (ForwardEuler: t_k + dt).  An advance of n steps adds n to k_first.
 * It is the handle's one clock: the atmospheric record below (swe2d_atm_*) is evaluated by it too, with or without a tide table, and
 * it advances once per step whichever of the two is present. */
int  swe2d_tide_clock(swe2d_handle *h, double t_base, int64_t k_first);
/* One launch at an explicit time (asynchronous): what the step-by-step path calls before swe2d_solve_stage. */
int  swe2d_tide_eval(swe2d_handle *h, double t);
/* The values the elevation planes hold for the listed facets, out[n_facets][2].  Synchronous. */
int  swe2d_tide_read(swe2d_handle *h, double *out);

/* ---- Atmospheric forcing from a record of snapshots (thetis/forcing.py, AtmosphericForcingInterpolator.set_fields): 10 m wind and
 * mean-sea-level pressure per mesh vertex at n_times instants, interpolated linearly in time and turned into wind stress,
 *     x = (1 - alpha)*x_j + alpha*x_{j+1}  for u, v, p,     j the largest index with times[j] <= t (at most n_times - 2),
 *     alpha = (t - times[j])/(times[j+1] - times[j])       (within 1e-6 outside [0, 1]: clamped; further out: SWE2D_ERR_INVALID_ARGUMENT)
 *     m = sqrt(u*u + v*v),  tau = C_D(m)*SWE2D_ATM_RHO_AIR*m,  tau_x = tau*u,  tau_y = tau*v
 *     LARGE_YEAGER_2009: C_D = 1e-3*(2.7/(m + 1e-3) + 0.142 + m/13.09 - 3.14807e-10*m6), m6 = (m*m)*(m*m)*(m*m); 2.34e-3 where m > 33
 *     LARGE_POND_1981:   C_D = 1.2e-3; 1e-3*(0.49 + 0.065*m) where m > 11          SMITH_BANKE_1975: C_D = (0.63 + 0.066*m)/1000
 * formed left to right without contraction, written into the planes of SWE2D_FIELD_WIND_STRESS and SWE2D_FIELD_ATMOSPHERIC_PRESSURE of
 * every cell (the continuous P1 injection of swe2d_set_field_vertex).  A handle with a record steps like one with a tide table: stage
 * launches, one evaluation launch in front of each (after the tide's, if any) at the time of the clock (swe2d_tide_clock), all enqueued
 * by the one swe2d_advance / swe2d_advance_forward_euler / swe2d_advance_coupled call; the fused and the dataflow kernels decline it
 * (the *_info calls and swe2d_flow_supported report 0; swe2d_solve_flow, swe2d_solve_step_cells, swe2d_solve_stage_pair_cells and
 * per-launch swe2d_advance_timed return SWE2D_ERR_UNSUPPORTED).  An advance one of whose stage times lies outside the record fails
 * with SWE2D_ERR_INVALID_ARGUMENT before anything is enqueued: the state and the clock are untouched.  The time is a kernel argument:
 * inside a stream capture those advances and every swe2d_atm_* call return SWE2D_ERR_UNSUPPORTED.  No reference counterpart at the C
 * level. */
#define SWE2D_ATM_WIND 1
#define SWE2D_ATM_PRESSURE 2
#define SWE2D_ATM_LARGE_YEAGER_2009 0
#define SWE2D_ATM_LARGE_POND_1981 1
#define SWE2D_ATM_SMITH_BANKE_1975 2
#define SWE2D_ATM_RHO_AIR 1.22
/* Sets (or replaces) the record, all of it resident on the device: times[n_times] strictly increasing (n_times >= 2), wind_u, wind_v,
 * pressure [n_times][n_vertices] in the numbering of swe2d_mesh.vertex_xy, all finite; `which` = SWE2D_ATM_WIND | SWE2D_ATM_PRESSURE
 * names the quantities forced (the tables of the other may be NULL), `method` the stress formulation.  Allocates the planes of the
 * forced fields if absent.  An allocation failure (SWE2D_ERR_HIP, the message names the bytes asked for) leaves the handle as it was. */
int  swe2d_atm_set(swe2d_handle *h, int32_t n_times, const double *times, const double *wind_u, const double *wind_v,
                   const double *pressure, int32_t method, int32_t which);
/* Drops the record; the planes keep their last values (swe2d_set_field(h, field, NULL) frees them). */
int  swe2d_atm_clear(swe2d_handle *h);
/* One launch at an explicit time (asynchronous): what the step-by-step path calls before swe2d_solve_stage. */
int  swe2d_atm_eval(swe2d_handle *h, double t);
/* What the planes of the two fields hold, in the nodal layout of swe2d_set_field: wind_nodal[n_cells][nodes_per_cell][2],
 * pressure_nodal[n_cells][nodes_per_cell]; either may be NULL.  Synchronous. */
int  swe2d_atm_read(swe2d_handle *h, double *wind_nodal, double *pressure_nodal);

/* ---- Running field statistics: extrema, means and harmonic sums of the whole state over every sampled step.
 * A statistics set holds 8 + 2K accumulators per DG node (K harmonic constituents, 0 <= K <= SWE2D_MAX_TIDE_CONSTITUENTS) in planes
 * laid out like the state.  One sample takes e, u, v of every node as swe2d_get_state returns them (wetting-drying: eta, not the
 * displaced depth) and updates, left to right without contraction,
 *     q = u*u + v*v,  s = sqrt(q)
 *     0: e_min = e < e_min ? e : e_min     1: e_max = e > e_max ? e : e_max     2: q_max = q > q_max ? q : q_max
 *     3: e_sum += e    4: u_sum += u    5: v_sum += v    6: s_sum += s    7: s3_sum += q*s
 *     8 + 2k: C_k += e*wc_k        9 + 2k: S_k += e*ws_k
 * with the weights wc_k = cos(omega_k t), ws_k = sin(omega_k t) formed by the CALLER: the device evaluates no transcendental, and all
 * accumulators but s_sum / s3_sum (the device's sqrt) have the bits of the same expressions evaluated on the host.  A new or reset
 * set holds e_min = +inf, e_max = q_max = -inf and zeros.  Every statistics call inside a stream capture returns
 * SWE2D_ERR_UNSUPPORTED.  No reference counterpart (the reference's AccumulatorCallback integrates a scalar in time, not fields). */
int  swe2d_stats_create(swe2d_handle *h, int32_t n_constituents, int32_t *stats_id);
/* one sample of the current state: ONE launch on the handle's stream, no synchronisation.  weights [2K]: wc_0, ws_0, wc_1, ...;
 * may be NULL when K = 0 */
int  swe2d_stats_append(swe2d_handle *h, int32_t stats_id, const double *weights);
/* synchronises; out [8 + 2K][n_cells][nodes_per_cell] in the handle's cell numbering, n_samples = appends since create / reset.
 * Does not clear. */
int  swe2d_stats_read(swe2d_handle *h, int32_t stats_id, double *out, int64_t *n_samples);
int  swe2d_stats_reset(swe2d_handle *h, int32_t stats_id);
int  swe2d_stats_destroy(swe2d_handle *h, int32_t stats_id);

/* ---- Lagrangian particle tracking: drifters advected in the velocity field of the state, one explicit-midpoint move per call.
 * A particle set holds N particles: position (double x, y), cell (the handle's own numbering), status, the marker it left through,
 * a wall-hit counter, and `capacity` rows [N][2] of recorded positions.  Triangles only (SWE2D_ERR_UNSUPPORTED on quadrilaterals).
 * swe2d_particles_advance is ONE launch on the handle's stream, no synchronisation: every ACTIVE particle makes, in the velocity of
 * buffer A frozen over the move and left to right without contraction (only + - * / and comparisons: a host replay has its bits),
 *     u1 = U(x, k);   (xm, km) = probe(x, k, (0.5*dt_move)*u1);   u2 = U(xm, km);   (x', k') = move(x, k, dt_move*u2)
 * U(x, k): with the cell's vertices p0, p1, p2:  a = p1 - p0, b = p2 - p0, det = a.x*b.y - b.x*a.y, d = x - p0,
 *     l1 = (d.x*b.y - b.x*d.y)/det,  l2 = (a.x*d.y - d.x*a.y)/det,  l0 = (1 - l1) - l2,   U = (l0*u0 + l1*u1) + l2*u2 per component.
 *     The coordinate that vanishes on facet f (which joins the local vertices f, f + 1) is m_f = l_((f + 2) % 3).
 * move(x, k, d): the straight walk along x -> y = x + d.  In the current cell form m_f(x), m_f(y).  The candidates are the facets
 *     with m_f(y) < 0, the facet just entered through excepted; without a candidate the particle arrives at (y, cell).  Else the
 *     candidate of the smallest s_f = m_f(x)/(m_f(x) - m_f(y)) is crossed (ties: the lowest f): an interior facet continues in the
 *     neighbour; a boundary facet whose marker is open sets EXITED, stores the marker and freezes the particle at x + s*d; any other
 *     boundary is a wall: the particle arrives at x + (s*(1 - 2^-10))*d in that cell, stays ACTIVE, its wall-hit counter goes up by one.
 *     A walk that has not arrived within SWE2D_PARTICLE_MAX_HOPS cells makes the particle LOST at its position before the advance (a
 *     bound on the loop, not a tolerance).  probe() is the same walk without consequences: an open boundary or a wall only ends it,
 *     at the crossing point or the shortened point; a probe that does not arrive makes the particle LOST as well.
 * EXITED and LOST particles are never touched again.  Every call inside a stream capture returns SWE2D_ERR_UNSUPPORTED.  No reference
 * counterpart (the reference has no 2D particle tracker). */
#define SWE2D_PARTICLE_ACTIVE 0
#define SWE2D_PARTICLE_EXITED 1
#define SWE2D_PARTICLE_LOST 2
#define SWE2D_PARTICLE_MAX_HOPS 64
/* xy [n][2], cells [n]: every cell in range and every position inside its cell (all three coordinates >= -1e-12), else
 * SWE2D_ERR_INVALID_ARGUMENT; capacity >= 0 rows.  An allocation failure (SWE2D_ERR_HIP, the message names the bytes asked for)
 * leaves the handle as it was. */
int  swe2d_particles_create(swe2d_handle *h, int32_t n_particles, const double *xy, const int32_t *cells, int32_t capacity,
                            int32_t *particles_id);
/* one move of every ACTIVE particle (asynchronous); open_markers [n_open], n_open <= SWE2D_MAX_MARKERS, each in 1..SWE2D_MAX_MARKERS-1 */
int  swe2d_particles_advance(swe2d_handle *h, int32_t particles_id, double dt_move, int32_t n_open, const int32_t *open_markers);
/* the current positions as one more row (asynchronous); SWE2D_ERR_INVALID_ARGUMENT and nothing written when the set holds `capacity` rows */
int  swe2d_particles_record(swe2d_handle *h, int32_t particles_id);
/* synchronises; xy [n][2], cells, status, exit_markers (0: none), wall_hits [n]; any of them may be NULL */
int  swe2d_particles_read(swe2d_handle *h, int32_t particles_id, double *xy, int32_t *cells, int32_t *status, int32_t *exit_markers,
                          int32_t *wall_hits);
/* the rows recorded since the last read -> out [rows][n][2] (room for `capacity` rows), then the row buffer is empty */
int  swe2d_particles_read_rows(swe2d_handle *h, int32_t particles_id, double *out, int32_t *n_rows);
int  swe2d_particles_destroy(swe2d_handle *h, int32_t particles_id);
/* ---- Opt-in per particle set: random-walk dispersion, timed releases, cell counts.  A set that uses none of them is advanced by
 * swe2d_particles_advance as before.  swe2d_particles_advance_at is the same ONE launch with the time `t` at which the move ends; it
 * counts the set's moves (the counter starts at 0 with the set).
 * Timed releases: a WAITING particle sits at its release position and turns ACTIVE in the first move with t - dt_move >= its release
 *     time, which moves it already.
 * Random walk (Visser 1997, uniform deviates), after a midpoint move that arrived or ended at a wall, at (x', k'), dt = dt_move, left
 *     to right without contraction: K0, K1, K2 the diffusivity at the vertices of k', l0, l1, l2 the coordinates of x' as above,
 *         Kx = (l0*K0 + l1*K1) + l2*K2;   gx = ((K1-K0)*b.y - (K2-K0)*a.y)/det;   gy = (a.x*(K2-K0) - b.x*(K1-K0))/det
 *         Ko = Kx + (0.5*dt)*(gx*gx + gy*gy), a negative Ko is 0;   amp = sqrt((6.0*dt)*Ko)   (the correctly rounded square root)
 *         d = (dt*gx + amp*Rx, dt*gy + amp*Ry);   (x'', k'') = move(x', k', d)   unless d is (0, 0), which is no walk
 *     An open boundary: EXITED at the crossing; a wall: stopped at the shortened point, one more wall hit (a move can count two), no
 *     reflection; SWE2D_PARTICLE_MAX_HOPS reached: LOST at the position before the whole advance, nothing else written.
 *     (w0, w1, w2, w3) = Philox4x32-10(counter = (particle index, moves made before, 0, 0), key = (seed & 0xffffffff, seed >> 32)),
 *     multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85;
 *         Rx = 2*(((w0 >> 5)*67108864.0 + (w1 >> 6))*2^-53) - 1,   Ry the same of w2, w3: in [-1, 1), every operation exact. */
#define SWE2D_PARTICLE_WAITING 3
/* diffusivity [n_vertices] at the vertices (the numbering of swe2d_mesh.vertex_xy), finite and >= 0, n_vertices that of the mesh,
 * else SWE2D_ERR_INVALID_ARGUMENT; from now on swe2d_particles_advance_at adds the random walk; synchronises */
int  swe2d_particles_set_diffusivity(swe2d_handle *h, int32_t particles_id, int32_t n_vertices, const double *diffusivity, uint64_t seed);
/* release_times [n] (n that of the set, no NaN; +-infinity allowed): ACTIVE and WAITING particles become WAITING where
 * release_times[p] > t_now and ACTIVE elsewhere; from now on swe2d_particles_advance_at runs the release gate; synchronises */
int  swe2d_particles_set_release_times(swe2d_handle *h, int32_t particles_id, int32_t n, const double *release_times, double t_now);
/* one move that ends at time t (asynchronous); arguments as swe2d_particles_advance; dt_move >= 0 for a set with a diffusivity */
int  swe2d_particles_advance_at(swe2d_handle *h, int32_t particles_id, double dt_move, double t, int32_t n_open, const int32_t *open_markers);
/* counts [n_cells] (the handle's own numbering): the particles in every cell whose status s has bit s of status_mask set - one
 * small launch of 32-bit integer atomic adds into a zeroed buffer of the set, so the result does not depend on the order; synchronises */
int  swe2d_particles_cell_counts(swe2d_handle *h, int32_t particles_id, uint32_t status_mask, int32_t *counts);

/* ---- Reacting tracers: a tracer's source as an expression of tracer fields, evaluated in front of every stage of that tracer.
 * The source term of the reference is inner(source, test)*dx with the live Functions (tracer_eq_2d.py:281-298).  Here a tracer
 * may carry a PROGRAM: postfix code on a stack of doubles, one int32 word per instruction, op | arg << 8.  Every launch of a stage of
 * that tracer (swe2d_tracer_solve_stage[_cells], swe2d_tracer_forward_euler, swe2d_tracer_tendency, swe2d_advance_coupled) is preceded by
 * ONE launch over the same cell range that writes the tracer's nodal source planes (what swe2d_tracer_set_source uploads otherwise);
 * the stage kernels are the ones of a sourced tracer.  Per cell, left to right without contraction:
 *   1. at point q of the rule (phi [n_q][nodes_per_cell], w [n_q], weights summing to 1 on the reference cell) an operand with the
 *      cell's nodal values c is  (phi[q][0]*c[0] + phi[q][1]*c[1]) + phi[q][2]*c[2]  (quadrilaterals: ... + phi[q][3]*c[3]); X and Y
 *      are the operands whose nodal values are the cell's vertex coordinates
 *   2. the program gives s_q
 *   3. from b = 0:  b_i = b_i + (w[q]*phi[q][i])*s_q  for q ascending
 *   4. the nodal source is the reference cell's mass inverse applied to b (the constant Jacobian cancels):
 *      triangles  12*b_i - 3*((b_0 + b_1) + b_2);   parallelograms  (16*b_i - 8*(b_(i+1) + b_(i+3))) + 4*b_(i+2), indices mod 4.
 * Instructions (a, b: the two topmost values, b on top; every leaf pushes one value):
 *   CONST i   consts[i]                      TRACER j  tracer j: during a stage of tracer `tracer_id` operand TRACER tracer_id is that
 *   FIELD f   coefficient field of slot f              stage's INPUT buffer, every other tracer its buffer A (already stepped for lower
 *   X, Y      coordinates                              ids, old for higher ids: the Gauss-Seidel order of swe2d_advance_coupled)
 *   ADD a + b   SUB a - b   MUL a*b   DIV a/b   NEG -a   ABS |a|   MIN b < a ? b : a   MAX b > a ? b : a
 *   POWI n    2 <= n <= 16:  r = a;  r = r*a  repeated n - 1 times
 *   SQRT EXP LOG   the device's math library (SQRT is correctly rounded; EXP and LOG need not round as a host library does)
 *   LT LE GT GE EQ NE   a op b ? 1.0 : 0.0      AND  a != 0 && b != 0     OR  a != 0 || b != 0     NOT  a == 0   (1.0 / 0.0)
 *   SELECT    of the three topmost values c, a, b (b on top):  c != 0 ? a : b
 * A conservative tracer's operand is the stored field q = H*T (and the stage kernel multiplies the source by H as for any source).
 * Limits: SWE2D_REACTION_MAX_CODE instructions, at most SWE2D_REACTION_MAX_STACK values on the stack at any time (the program is
 * checked when it is set: no underflow, exactly one value left), SWE2D_REACTION_MAX_CONSTS constants, SWE2D_REACTION_MAX_FIELDS
 * coefficient fields per handle, SWE2D_REACTION_MAX_TRACERS distinct tracers per program, SWE2D_REACTION_MAX_QUAD points.
 * Triangles and parallelograms only: SWE2D_ERR_UNSUPPORTED on a handle with general quadrilaterals. */
#define SWE2D_REACTION_MAX_CODE 64
#define SWE2D_REACTION_MAX_STACK 8
#define SWE2D_REACTION_MAX_CONSTS 16
#define SWE2D_REACTION_MAX_FIELDS 4
#define SWE2D_REACTION_MAX_TRACERS 8
#define SWE2D_REACTION_MAX_QUAD 64
enum swe2d_reaction_op {
    SWE2D_RX_CONST = 0, SWE2D_RX_TRACER, SWE2D_RX_FIELD, SWE2D_RX_X, SWE2D_RX_Y,
    SWE2D_RX_ADD, SWE2D_RX_SUB, SWE2D_RX_MUL, SWE2D_RX_DIV, SWE2D_RX_NEG, SWE2D_RX_ABS, SWE2D_RX_MIN, SWE2D_RX_MAX, SWE2D_RX_POWI,
    SWE2D_RX_SQRT, SWE2D_RX_EXP, SWE2D_RX_LOG,
    SWE2D_RX_LT, SWE2D_RX_LE, SWE2D_RX_GT, SWE2D_RX_GE, SWE2D_RX_EQ, SWE2D_RX_NE, SWE2D_RX_AND, SWE2D_RX_OR, SWE2D_RX_NOT, SWE2D_RX_SELECT,
    SWE2D_RX_COUNT
};
/* sets (n_code > 0) or removes (n_code = 0: the tracer has no source again) the program of a tracer.  The source planes are allocated
 * here; an allocation failure names the bytes.  swe2d_tracer_set_source on the tracer replaces the program by the uploaded source. */
int  swe2d_tracer_set_reaction(swe2d_handle *h, int tracer_id, int32_t n_code, const int32_t *code, int32_t n_const,
                               const double *consts, int32_t n_q, const double *phi, const double *w);
/* new values for the constants of the tracer's program (n_const as set) */
int  swe2d_tracer_set_reaction_constants(swe2d_handle *h, int tracer_id, int32_t n_const, const double *consts);
/* coefficient field of slot 0 .. SWE2D_REACTION_MAX_FIELDS-1: nodal [n_cells][nodes_per_cell]; NULL frees the slot.  A stage of a
 * tracer whose program names an empty slot returns SWE2D_ERR_INVALID_ARGUMENT. */
int  swe2d_reaction_set_field(swe2d_handle *h, int32_t slot, const double *nodal);
/* synchronises; the tracer's nodal source planes [n_cells][nodes_per_cell] as the last pass (or swe2d_tracer_set_source) left them;
 * SWE2D_ERR_INVALID_ARGUMENT for a tracer without a source */
int  swe2d_tracer_get_source(swe2d_handle *h, int tracer_id, double *nodal);
/* synchronises; tracer buffer i_buffer = 0 (T0 / the step result), 1 or 2 (what stages 0 and 1 wrote) [n_cells][nodes_per_cell]: what
 * a host evaluation of a reacting source reads between the stages */
int  swe2d_tracer_get_buffer(swe2d_handle *h, int tracer_id, int i_buffer, double *nodal);

/* ---- Suspended sediment and Exner bed evolution (triangles, whole meshes, no wetting-drying).
 * One tracer of the handle is the sediment field S (conservative form: q = H*S).  Its source is not uploaded: a pass in front of every
 * stage launch of that tracer writes it from three sets of nodal planes - erosion flux E, deposition coefficient D, equilibrium
 * concentration - that swe2d_sediment_update evaluates from buffer A, ONCE per time step (frozen over the stages, as the reference's
 * SedimentModel.update(), coupled_timeintegrator_2d.py:100-135).
 * Closures (thetis/sediment_model.py:136-211), evaluated at the three DG nodes of a cell from that cell's own nodal (u, v) and
 * H = eta + bathymetry (linear equations: H = bathymetry) - the reference projects uv and H into CG-P1 first; this is the stated
 * difference.  With the parameters below, every comparison a select:
 *   U2 = u*u + v*v;  hc = max(H, 0.001);  qfc = 2/(log(max(11.036*hc/ks, 1.001))/kappa)^2
 *   cfactor = H > ksp ? 2/((1/kappa)*log(11.036*H/ksp))^2 : 0;  mu = qfc > 0 ? cfactor/qfc : 0
 *   B = a > H ? 1 : a/H;  ustar = sqrt(0.5*qfc*U2);  rouse = ws/(kappa*ustar) - 1;  rm = min(rouse, 3)
 *   step = |rouse| > 1e-4 ? B*(1 - pow(B, rm))/rm : -B*log(B);  integrated_rouse = max(step > 1e-12 ? 1/step : 1e12, 1)
 *   tau = rho0*0.5*qfc*U2*mu;  T = tau > 0 ? (tau - taucr)/taucr : -1;  T15 = T > 0 ? T*sqrt(T) : 0
 *   E = ws*(erosion_factor*T15);  D = ws*integrated_rouse;  equilibrium = E/D
 * log / pow / sqrt are the device's math library.  The remaining passes are + - * / in the order written, without contraction:
 *   source (per stage, S the stage's input buffer, H from buffer A and the current bed):   s = (E - D*S)/H;  conservative  s = E - (D*q)/H
 *     - the nodal interpolant of the reference's erosion and deposition terms (sediment_eq_2d.py:84-104), not their projection
 *   'equilibrium' boundary (with the update): the per-facet value table of the tracer (swe2d_tracer_set_bc_facets) takes, on the
 *     facets of the markers set by swe2d_sediment_set_equilibrium_bc, the cell's own equilibrium value at each of its nodes -
 *     conservative form: times that node's H (the inner depth: the reference's value for a boundary dict without 'elev')
 *   Exner (swe2d_exner_step, lumped CG-P1 form of exner_eq.py:68-84; bathymetry positive downwards, erosion deepens): per vertex v,
 *     over its (cell c, local node i) pairs in ascending cell order, j = (i+1)%3, k = (i+2)%3, r = E - D*S [conservative E - (D*q)/H]:
 *       num = num + (A_c/12)*((2*r_i + r_j) + r_k);   den = den + A_c/3;   A_c = 0.5*|(x1-x0)*(y2-y0) - (x2-x0)*(y1-y0)|
 *       b_v = b_v + ((dt*fac)*num)/den
 *     A vertex where min over its nodes of (eta + new b) [linear equations: new b] falls below min_depth keeps its bed and is counted
 *     (swe2d_exner_skipped).  A right-hand side that does not depend on the bed and a lumped mass: ForwardEuler and SSPRK33 are
 *     this same single update.
 * swe2d_advance_coupled steps, per time step: the flow, every other tracer, swe2d_sediment_update, the three sediment stages, the
 * limiter, and with solve_exner the bed update.  The dataflow kernel, which batches steps, declines a handle with solve_exner. */
typedef struct swe2d_sediment_params {
    double ws;               /* settling velocity */
    double dstar;            /* dimensionless grain size (carried for reference; erosion_factor holds its power) */
    double taucr;            /* critical bed shear stress */
    double a;                /* bed_reference_height/2 */
    double ksp;              /* grain roughness 3*d50 */
    double ks;               /* bed_reference_height */
    double rho0;
    double kappa;            /* von Karman */
    double fac;              /* morphological_acceleration_factor/(1 - porosity) */
    double erosion_factor;   /* 0.015*(d50/a)/dstar^0.3 */
    double min_depth;        /* floor of the depth in the Exner update, > 0 */
    int32_t conservative;    /* the tracer holds q = H*S */
    int32_t solve_exner;     /* swe2d_advance_coupled updates the bed after the sediment step */
} swe2d_sediment_params;
/* makes tracer `tracer_id` the sediment field (allocates its source planes, the coefficient planes and the Exner tables; sets the
 * tracer's conservative flag).  The tracer must have neither an uploaded source nor a reaction program (SWE2D_ERR_INVALID_ARGUMENT);
 * while it is the sediment field swe2d_tracer_set_source and swe2d_tracer_set_reaction on it are refused (removing: no-ops), and
 * swe2d_sediment_clear gives back a plain tracer without a source in the non-conservative form.  SWE2D_ERR_UNSUPPORTED: quadrilaterals, partitions, wetting-drying, solve_exner with turbine farms. */
int  swe2d_sediment_set(swe2d_handle *h, int tracer_id, const swe2d_sediment_params *par);
/* marker slot 1 .. SWE2D_MAX_MARKERS-1 of the sediment tracer carries 'equilibrium' (on = 0: no longer) */
int  swe2d_sediment_set_equilibrium_bc(swe2d_handle *h, int marker, int on);
/* E, D, equilibrium from buffer A and the current bed; the 'equilibrium' facets of the value table (asynchronous) */
int  swe2d_sediment_update(swe2d_handle *h);
/* synchronises; the planes as nodal [n_cells][3]; any pointer may be NULL */
int  swe2d_sediment_read(swe2d_handle *h, double *erosion, double *deposition, double *equilibrium);
/* synchronises; the sediment tracer's per-facet value table [facet 3][n_cells][node 3] */
int  swe2d_sediment_read_bc(swe2d_handle *h, double *facet_nodal);
/* the tracer is a plain tracer without a source again; the tables are freed */
int  swe2d_sediment_clear(swe2d_handle *h);
/* one bed update from the sediment tracer's buffer A with the handle's dt (asynchronous).  With a bedload model the contribution
 * planes of the last swe2d_bedload_update are added; a handle with bedload and no sediment field is updated from them alone, and
 * swe2d_exner_skipped counts for it too */
int  swe2d_exner_step(swe2d_handle *h);
/* synchronises; vertices left unchanged by the bed updates since swe2d_sediment_set */
int  swe2d_exner_skipped(swe2d_handle *h, int64_t *n_skipped);
/* synchronises; the bathymetry [n_vertices] as the kernels read it */
int  swe2d_get_bathymetry(swe2d_handle *h, double *vertex_values);
/* synchronises; replaces the bathymetry [n_vertices] (every kernel reads it at launch).  SWE2D_ERR_UNSUPPORTED with wetting-drying */
int  swe2d_set_bathymetry(swe2d_handle *h, const double *vertex_values);

/* ---- Bedload transport in the Exner update (thetis/sediment_model.py:213-310 get_bedload_term, thetis/exner_eq.py:87-129), in this
 * build's formulation: nodal closures from the cell's own DG values, lumped CG-P1 Exner, an explicit bed - the reference's "new"
 * bathymetry in slopecoef, calfamod and the secondary current is the old one, so ForwardEuler and SSPRK33 of the Exner stepper stay the
 * same single update.  With or without a sediment field (swe2d_sediment_set) on the handle.
 * Nodal transport q_b = (qbx, qby), per cell k and local node i from the node's (u, v), H = eta + h (linear equations: h) and the
 * cell-constant gradients of the bed and of the free surface, j over the cell's nodes in order, d psi_j the gradient table below:
 *   hx = (h_0*dpsi_0x + h_1*dpsi_1x) + h_2*dpsi_2x, hy likewise;  (ex, ey) the same of eta_j (linear equations: 0, as the reference's
 *   depth_tot.dx - bathymetry.dx vanishes).  Every comparison a select, no contraction, g the handle's g_grav:
 *   U2, qfc, mu as for the suspended load above (one function in the kernels)
 *   stress = rho0*0.5*qfc*U2;  thetaprime = mu*stress/shields_den;  moves = thetaprime > thetacr
 *   x = moves ? thetaprime - thetacr : 0;  phi = moves ? 8*x*sqrt(x) : 0;  sn = moves ? sqrt(U2) : 1;  calfa = u/sn;  salfa = v/sn
 *   magnitude correction:  slopecoef = 1 + beta*(hx*calfa + hy*salfa)            [off: 1; not clipped, as in the reference]
 *   angle correction:      cparam = shields_den*(surbeta2*surbeta2);  tt1 = sqrt(cparam/max(stress, 1e-10))
 *                          aa = salfa + tt1*hy;  bb = calfa + tt1*hx;  nrm = max(sqrt(aa*aa + bb*bb), 1e-10);  (ca, sa) = (bb, aa)/nrm
 *                                                                                 [off: (ca, sa) = (calfa, salfa)]
 *   secondary current:     vs = u*ey - v*ex;  tdf = 7*g*rho0*H*qfc/(2*alpha_secc*(moves ? U2 : 1))
 *                          t1 = stress*slopecoef*ca + v*tdf*vs;  t2 = stress*slopecoef*sa - u*tdf*vs;  t4 = sqrt(t1*t1 + t2*t2)
 *                          factor = t4/(moves ? stress : 1);  (ca, sa) = (t1, t2)/(t4 > 0 ? t4 : 1)     [off: factor = slopecoef]
 *   q_b = (factor*phi*qb_scale)*(ca, sa)  where phi > 0 (and, with the secondary current, t4 > 0);  (0, 0) exactly elsewhere -
 *   water at rest included, where the reference's u/sqrt(U2) is 0/0.  Products and quotients associate from the left.
 * Divergence: q_b is the P1 interpolant of its nodal values in the cell.  The contribution of cell k to its node i is
 *   c_i = -(A*(mx*dpsi_ix + my*dpsi_iy)),  mx = ((qbx_0 + qbx_1) + qbx_2)/3, my likewise, and then, for the facets f = 0, 1, 2 of the
 *   cell in order (facet f joins the nodes a = f and b = (f+1)%3, o = (f+2)%3 opposite) that lie on an OPEN marker, with
 *   N = (-((2*A)*dpsi_ox), -((2*A)*dpsi_oy)) = length * outward normal:
 *     c_a = c_a + ((2*qbx_a + qbx_b)*Nx + (2*qby_a + qby_b)*Ny)/6;   c_b = c_b + ((2*qbx_b + qbx_a)*Nx + (2*qby_b + qby_a)*Ny)/6
 *   Interior facets contribute nothing (the test space is continuous); a closed boundary facet contributes nothing (no transport through it).
 *   Gradient table, built by the host part of the library without contraction, det = (x1-x0)*(y2-y0) - (x2-x0)*(y1-y0):
 *     dpsi_0 = ((y1-y2)/det, (x2-x1)/det);  dpsi_1 = ((y2-y0)/det, (x0-x2)/det);  dpsi_2 = ((y0-y1)/det, (x1-x0)/det)
 * Exner with bedload: the gather adds nb = sum of c_{k,i} over the vertex's list, separately, and  b_v = b_v + ((dt*fac)*(num + nb))/den
 *   (exner_eq.py:127-129: bathymetry positive downwards, a positive divergence of q_b deepens the bed); without a sediment field num = 0.
 *   A handle without bedload executes (dt*fac)*num/den as before.  With the magnitude correction the update is diffusive in h and explicit:
 *   dt*fac is bounded by the caller.
 * Per time step (swe2d_advance_coupled, and swe2d_advance for a handle with bedload and solve_exner): flow, tracers, sediment stages,
 * limiter, swe2d_bedload_update, Exner.  The dataflow kernel declines a handle whose bed moves.  Every other entry that steps the flow
 * (swe2d_advance_forward_euler, swe2d_solve_stage and its variants, swe2d_solve_flow, swe2d_advance_timed per launch) steps the flow
 * alone and leaves the bed where it is: a caller of those issues swe2d_bedload_update and swe2d_exner_step itself. */
typedef struct swe2d_bedload_params {
    double beta;             /* slope_effect_parameter (magnitude correction) */
    double surbeta2;         /* slope_effect_angle_parameter */
    double alpha_secc;       /* secondary_current_parameter */
    double thetacr;          /* critical Shields parameter */
    double shields_den;      /* (rhos - rho0)*g*d50 */
    double qb_scale;         /* sqrt(g*R*d50^3) */
    double ks;               /* as swe2d_sediment_params: bed_reference_height */
    double ksp;              /* 3*d50 */
    double kappa;
    double rho0;
    double fac;              /* morphological_acceleration_factor/(1 - porosity): read by the Exner update of a handle without a sediment field */
    double min_depth;        /* likewise: floor of the depth in the Exner update, > 0 */
    int32_t use_slope_mag_correction;
    int32_t use_angle_correction;
    int32_t use_secondary_current;
    int32_t solve_exner;     /* swe2d_advance_coupled / swe2d_advance update the bed after every step */
    uint32_t open_markers;   /* bit m: boundary facets of marker slot m are open to the transport */
    int32_t fuse_with_sediment; /* 1: with a sediment field whose ks, ksp and kappa are these, swe2d_sediment_update writes q_b and the
                              * contributions in the coefficient pass's launch (friction closures once per node for both), and
                              * swe2d_advance_coupled has no bedload launch of its own - the same bits; 0 (the measured choice, DESIGN.md
                              * 5h): a launch of its own after the limiter */
} swe2d_bedload_params;
/* switches the bedload model on or replaces its parameters (allocates the q_b and contribution planes, the gradient table and, where
 * the handle has none yet, the Exner tables).  SWE2D_ERR_UNSUPPORTED: the cases of swe2d_sediment_set. */
int  swe2d_bedload_set(swe2d_handle *h, const swe2d_bedload_params *par);
/* q_b and the contribution planes from buffer A and the current bed (asynchronous) */
int  swe2d_bedload_update(swe2d_handle *h);
/* synchronises; the planes as nodal [n_cells][3]; any pointer may be NULL */
int  swe2d_bedload_read(swe2d_handle *h, double *qbx, double *qby, double *contrib);
/* no bedload in the Exner update any more; the planes are freed (and the Exner tables of a handle without a sediment field) */
int  swe2d_bedload_clear(swe2d_handle *h);

/* ---- Sediment slide in the Exner update (thetis/sediment_model.py:312-354 get_sediment_slide_term, thetis/exner_eq.py:132-149
 * ExnerSedimentSlideTerm): a diffusion of the bed that switches on in cells steeper than the angle of repose.  The bed is CG-P1, so
 * the three interior-facet integrals of the reference's term vanish (jump(b) = 0); what remains is  int grad(psi) . (alpha grad(-b)) dx
 * with residual = -f, alpha the cell-constant scalar below.  With or without a sediment field and a bedload model on the handle.
 * Per cell k, b_j the bed at the cell's vertices, d psi_j the gradient table of the bedload section, r_k the slide region (1 without
 * one), dt the handle's step; every comparison a select, no contraction, products and quotients associate from the left:
 *   bx = (b_0*dpsi_0x + b_1*dpsi_1x) + b_2*dpsi_2x, by likewise;   gx = r_k*bx;  gy = r_k*by
 *   s2      = gx*gx + gy*gy
 *   nz      = 1/sqrt(1 + s2)
 *   sinb    = sqrt(1 - nz*nz)
 *   tanbeta = sinb/nz
 *   beta    = asin(sinb)
 *   d       = tanbeta - tanphi
 *   qaval   = d > 0 ? ((1 - porosity)*0.5*(L*L)*d)/cos(beta*dt*morfac) : 0          [the reference's cosine, kept verbatim]
 *   alpha   = sinb > 0 ? -(qaval*(nz*nz))/sinb : 0                                   [the divisor is 1 where sinb == 0]
 *   c_i     = (A*alpha)*(dpsi_ix*bx + dpsi_iy*by)     [the UNscaled gradient, as in the reference: the region enters the slope test only]
 * sqrt and the divisions are correctly rounded; asin and cos are the device's math library.  c_0 + c_1 + c_2 = 0 up to rounding (the
 * hat gradients of a cell add up to zero): the lumped bed volume is conserved, and there is no boundary term.  alpha < 0 makes the
 * update a diffusion of b.
 * Exner with slide: the gather adds ns = sum of c_{k,i} over the vertex's list, separately and NOT scaled by fac (the reference does
 * not multiply this term by morfac/(1 - porosity)):
 *   b_v = b_v + ((dt*fac)*(num + nb) + dt*ns)/den        (num = 0 without a sediment field, nb = 0 without bedload)
 *   A handle without slide executes what it executed before.
 * Counted, not enforced: a cell is FLAGGED when alpha > 0 (the cosine went negative: anti-diffusion) or when
 *   ((dt*|alpha|)*3)*max_i(dpsi_ix*dpsi_ix + dpsi_iy*dpsi_iy) > 1, a sufficient per-cell bound for the lumped forward-Euler diffusion.
 *   swe2d_slide_flagged gives the running count of flagged cells over all passes since swe2d_slide_set.
 * The largest beta of the last pass is kept in one device word as an exact, order-independent maximum (swe2d_slide_max_angle).
 * Per time step (swe2d_advance_coupled, and swe2d_advance on a handle without a sediment field): flow, tracers, sediment stages,
 * limiter, bedload, swe2d_slide_update, Exner.  The dataflow kernel declines a handle with slide. */
typedef struct swe2d_slide_params {
    double tanphi;           /* tan(max_angle*pi/180), formed by the caller */
    double length_scale;     /* sed_slide_length_scale L, > 0 */
    double porosity;
    double morfac;           /* morphological_acceleration_factor (the cosine's argument) */
    double fac;              /* morfac/(1 - porosity): read by the Exner update of a handle with neither sediment field nor bedload */
    double min_depth;        /* likewise: floor of the depth in the Exner update, > 0 */
    int32_t solve_exner;     /* swe2d_advance_coupled / swe2d_advance update the bed after every step */
} swe2d_slide_params;
/* switches the slide on or replaces its parameters and region (allocates the alpha, beta and contribution planes and, where the handle
 * has none yet, the gradient table and the Exner tables); region_per_cell: [n_cells] or NULL (1 everywhere).  Clears the flagged
 * count.  SWE2D_ERR_UNSUPPORTED: the cases of swe2d_sediment_set. */
int  swe2d_slide_set(swe2d_handle *h, const swe2d_slide_params *par, const double *region_per_cell);
/* alpha, beta, the contribution planes, the maximum and the flagged count from the current bed (asynchronous) */
int  swe2d_slide_update(swe2d_handle *h);
/* synchronises; alpha [n_cells], beta [n_cells], contrib nodal [n_cells][3]; any pointer may be NULL */
int  swe2d_slide_read(swe2d_handle *h, double *alpha, double *beta, double *contrib);
/* synchronises; the largest beta (radians) of the last swe2d_slide_update, 0 before the first */
int  swe2d_slide_max_angle(swe2d_handle *h, double *beta_max);
/* synchronises; cells flagged by the passes since swe2d_slide_set */
int  swe2d_slide_flagged(swe2d_handle *h, int64_t *n_flagged);
/* no slide in the Exner update any more; the planes are freed (and the tables nothing else reads): the handle steps as one that
 * never had it */
int  swe2d_slide_clear(swe2d_handle *h);

/* ---- Section transports (csrc/swe2d_sections.hip; thetis_amd/sections.py): volume and tracer flux through lines ----
 * The reference has no 2D counterpart (its TransectCallback is 3D, thetis/callback.py:959).  A section is a list of PIECES; a piece
 * is a straight segment inside one cell (a cut of a polyline, or a boundary facet), handed in with its geometry resolved by the host:
 * the cell, the nodal weights w[q][i] of the cell's nodes at the two Gauss-Legendre points q of the piece, and N = (nx, ny) len/2,
 * n the unit normal the transport is counted along.  With L = sqrt(Nx Nx + Ny Ny) (= len/2, formed by the host part of the
 * library) a piece contributes, without contraction and with f_q = fma(w[q][k-1], f[k-1], ... fma(w[q][1], f[1], w[q][0] f[0])) for
 * f = u, v, eta, h, c_t:
 *     H_q = eta_q + h_q   (use_nonlinear_equations = 0: h_q)        F_q = H_q fma(u_q, Nx, v_q Ny)
 *     transport  F_0 + F_1          area  L (H_0 + H_1)          tracer t  fma(F_1, c_t1, F_0 c_t0)
 * h is the handle's current vertex bathymetry.  On triangles every factor is linear along a piece, so the two points integrate
 * int H u.n ds, int H ds, int H u.n c ds exactly; the same holds for a piece along an edge of a quadrilateral.  The terms of a
 * section are added as limb sums (swe2d_diagnostics_limbs): exact and independent of the order of the pieces.
 * A VALUE ROW is [SWE2D_MAX_SECTIONS][2 + SWE2D_MAX_SECTION_TRACERS]: transport, area, tracer 0 ..; a LIMB ROW has
 * SWE2D_SECTION_LIMBS int64 per value.  Slots without pieces and tracers not named are 0.  Terms that cannot be summed (not finite,
 * |x| >= 2^78) are left out and COUNTED per row; the count is handed out, it is not an error of the call.
 * SWE2D_ERR_UNSUPPORTED: a handle with wetting-drying; any of these calls inside a stream capture.  SWE2D_ERR_INVALID_ARGUMENT: a
 * cell outside 0 .. n_owned-1, a weight or normal that is not finite, a section slot or tracer id out of range, too many of either,
 * an append to a full row store.  The handle stays usable after either. */
#define SWE2D_MAX_SECTIONS 16
#define SWE2D_MAX_SECTION_TRACERS 4
#define SWE2D_SECTION_VALUES (2 + SWE2D_MAX_SECTION_TRACERS)
#define SWE2D_SECTION_LIMBS 6
/* replaces the handle's sections (synchronises).  piece_section[n_pieces] in 0 .. n_sections-1 (any order; n_sections <=
 * SWE2D_MAX_SECTIONS), piece_cell[n_pieces], piece_weights[n_pieces][2][nodes_per_cell], piece_normal[n_pieces][2],
 * tracer_ids[n_tracers] (n_tracers <= SWE2D_MAX_SECTION_TRACERS; may be NULL when 0).  Empties the row store. */
int  swe2d_sections_set(swe2d_handle *h, int32_t n_sections, int32_t n_pieces, const int32_t *piece_section, const int32_t *piece_cell,
                        const double *piece_weights, const double *piece_normal, int32_t n_tracers, const int32_t *tracer_ids);
int  swe2d_sections_clear(swe2d_handle *h);
/* the state now (buffer A), synchronously: one launch.  limbs [SWE2D_MAX_SECTIONS][SWE2D_SECTION_VALUES][SWE2D_SECTION_LIMBS] /
 * values [SWE2D_MAX_SECTIONS][SWE2D_SECTION_VALUES] = swe2d_sum_limbs_to_double of them; *n_unsummable: terms left out */
int  swe2d_sections_eval_limbs(swe2d_handle *h, int64_t *limbs, int64_t *n_unsummable);
int  swe2d_sections_eval(swe2d_handle *h, double *values, int64_t *n_unsummable);
/* rows kept on the device: reserve `capacity` rows (empties the store); append enqueues the one launch on the handle's stream (no
 * synchronisation, no host read); read synchronises, hands out the rows appended since the last read as values[n_rows][..] with
 * n_unsummable[n_rows] (either may be NULL) and empties the store */
int  swe2d_sections_rows_reserve(swe2d_handle *h, int32_t capacity);
int  swe2d_sections_rows_append(swe2d_handle *h);
int  swe2d_sections_rows_read(swe2d_handle *h, double *values, int64_t *n_unsummable, int32_t *n_rows);

/* ---- Smagorinsky eddy viscosity (csrc/swe2d_smag.hip; thetis_amd/smagorinsky.py) ----
 * The closure of thetis/utility3d.py:879-997 (SmagorinskyViscosity), whose formula is two-dimensional.  Per triangle K with area A:
 *  (1) the weak gradient g[c][x] in P1(K) of velocity component c in direction x (the reference's weak_form branch):
 *      M g = -int_K d_x phi_i u_c dx + sum_f int_f u_hat phi_i n_x ds, M the P1 mass matrix, u_hat the mean of the two traces on an
 *      interior facet and the own trace on every boundary facet, all integrals in closed form;
 *  (2) at the 6 points q of the degree-4 rule: D_T = g[0][0] - g[1][1], D_S = g[0][1] + g[1][0], h_q the P1 element size,
 *      nu_q = (c_s h_q)^2 sqrt(D_T^2 + D_S^2); the cell moments b[i] = A sum_q w_q lambda_i(q) nu_q;
 *  (3) per vertex v the LUMPED projection nu_v = sum b[i] / sum A/3 over the (cell, node) pairs of v IN THE ORDER OF THE TABLE handed
 *      to swe2d_smag_set (the reference solves the consistent mass matrix);
 *  (4) nu_v = max(min_val, min(nu_v, max_v)), max_v = max_const where that is >= 0, else (1/120) h_v^2 / dt with the handle's
 *      dt at the time of the update; the stage kernels then read background + nu_v, the background being what swe2d_set_viscosity
 *      was or is given (a constant or a per-vertex field; 0 without one - the SIPG term is then on).
 * While the closure is on, swe2d_advance, swe2d_advance_forward_euler and swe2d_advance_coupled make the update in front of EVERY
 * step, from the state the step starts from; the viscosity is frozen over the step's stages.  The host-stepped entry points
 * (swe2d_solve_stage ...) read the viscosity of the last update.  No atomics: the result does not depend on scheduling.
 * SWE2D_ERR_UNSUPPORTED: quadrilaterals, a partition (n_owned != n_cells), wetting-drying, set / clear / read inside a stream
 * capture. */
#define SWE2D_SMAG_GRADIENT 0   /* out[n_cells][2][2][3]: component, direction, node.  Sets the debug flag: the cell pass runs once
                                   more on the current state and writes the gradient planes too */
#define SWE2D_SMAG_MOMENTS  1   /* out[n_cells][3] */
#define SWE2D_SMAG_NU       2   /* out[n_vertices]: the clipped closure viscosity */
#define SWE2D_SMAG_TOTAL    3   /* out[n_vertices]: background + closure, what the stage kernels read */
/* switches the closure on (or replaces its parameters) and makes one update (synchronises before it).  h_elem_vertex[n_vertices] finite;
 * vertex_cell_ptr[n_vertices + 1], vertex_cell_idx[3 n_cells]: per vertex its (cell << 2 | local node) entries, every pair once */
int  swe2d_smag_set(swe2d_handle *h, double c_s, const double *h_elem_vertex, double min_val, double max_const_or_negative,
                    const int32_t *vertex_cell_ptr, const int32_t *vertex_cell_idx);
/* switches it off (synchronises): the caller's viscosity, or none, is what it was */
int  swe2d_smag_clear(swe2d_handle *h);
/* one evaluation from the current state (buffer A) on the handle's stream; no synchronisation */
int  swe2d_smag_update(swe2d_handle *h);
/* synchronises; `which`: SWE2D_SMAG_* */
int  swe2d_smag_read(swe2d_handle *h, int which, double *out);

#ifdef __cplusplus
}
#endif
#endif /* SWE2D_H */
