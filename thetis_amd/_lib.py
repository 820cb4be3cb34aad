"""
ctypes binding of the C ABI declared in include/swe2d.h (libswe2d_hip.so).

There is deliberately no fallback: if the shared library is missing this raises, and if no HIP device is
visible ``swe2d_create`` fails with SWE2D_ERR_NO_DEVICE - the product never computes on the CPU.
"""
import ctypes
import os
import warnings

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('THETIS_AMD_LIB') or os.path.join(_HERE, 'libswe2d_hip.so')   # env: kernel A/B experiments

MAX_MARKERS = 16
BC_ELEV, BC_UV, BC_UN, BC_FLUX = 1, 2, 4, 8
BC_ELEV_FIELD, BC_UV_FIELD, BC_UN_FIELD, BC_FLUX_FIELD = 16, 32, 64, 128
FIELD_CORIOLIS, FIELD_ATMOSPHERIC_PRESSURE, FIELD_MOMENTUM_SOURCE, FIELD_VOLUME_SOURCE, FIELD_WIND_STRESS = 0, 1, 2, 3, 4
FIELD_LINEAR_DRAG, FIELD_QUADRATIC_DRAG, FIELD_MANNING_DRAG, FIELD_NIKURADSE = 5, 6, 7, 8
SCALAR_LINEAR_DRAG, SCALAR_QUADRATIC_DRAG, SCALAR_MANNING_DRAG, SCALAR_NORM_SMOOTHER, SCALAR_NIKURADSE = 0, 1, 2, 3, 4

IPC_HANDLE_BYTES = 64    # include/swe2d.h SWE2D_IPC_HANDLE_BYTES (sizeof(hipIpcMemHandle_t))
SUM_LIMBS = 6             # include/swe2d.h: limbs per order-independent sum (swe2d_diagnostics_limbs)
ABI_VERSION = 12         # include/swe2d.h SWE2D_ABI_VERSION
# include/swe2d.h swe2d_option
(OPT_FUSED_STAGES, OPT_FLOW, OPT_FLOW_WD, OPT_BND_INLINE, OPT_LDSX, OPT_ALTERNATE, OPT_COMPACT_IDX, OPT_VISC_FUSION, OPT_WALL_FAST,
 OPT_FLOW_POLL, OPT_FLOW_CAPACITY, OPT_FLOW_TIMEOUT_MS, OPT_P2P_TIMEOUT_MS, OPT_P2P_ZONE, OPT_ROCTX) = range(15)
OPT_COUNT = 15
SNAPSHOT_SLOTS = 2
MAX_FARMS, MAX_THRUST_TABLE = 8, 16   # include/swe2d.h SWE2D_MAX_FARMS, SWE2D_MAX_THRUST_TABLE
MAX_FARM_QUAD = 64                    # include/swe2d.h SWE2D_MAX_FARM_QUAD
MAX_TIDE_CONSTITUENTS = 32            # include/swe2d.h SWE2D_MAX_TIDE_CONSTITUENTS
ATM_WIND, ATM_PRESSURE = 1, 2         # include/swe2d.h SWE2D_ATM_*: the quantities of an atmospheric record
ATM_METHODS = {'LargeYeager2009': 0, 'LargePond1981': 1, 'SmithBanke1975': 2}     # include/swe2d.h SWE2D_ATM_<formulation>
ATM_RHO_AIR = 1.22                    # include/swe2d.h SWE2D_ATM_RHO_AIR
STATS_FIXED = 8                       # accumulators of a statistics set besides the 2 per constituent (csrc/swe2d_stats.hip)
PARTICLE_ACTIVE, PARTICLE_EXITED, PARTICLE_LOST = 0, 1, 2   # include/swe2d.h SWE2D_PARTICLE_*: status of a tracked particle
PARTICLE_WAITING = 3                  # include/swe2d.h SWE2D_PARTICLE_WAITING: a timed release that has not come yet
PARTICLE_MAX_HOPS = 64                # include/swe2d.h SWE2D_PARTICLE_MAX_HOPS: cells one walk may visit
MAX_SECTIONS, MAX_SECTION_TRACERS = 16, 4   # include/swe2d.h SWE2D_MAX_SECTIONS, SWE2D_MAX_SECTION_TRACERS
SECTION_VALUES = 2 + MAX_SECTION_TRACERS    # include/swe2d.h SWE2D_SECTION_VALUES: transport, area, one per tracer
SMAG_GRADIENT, SMAG_MOMENTS, SMAG_NU, SMAG_TOTAL = 0, 1, 2, 3   # include/swe2d.h SWE2D_SMAG_*: what swe2d_smag_read hands out
PROBE_UV, PROBE_ELEV = -1, -2  # include/swe2d.h SWE2D_PROBE_*: fields of a probe set (a tracer id >= 0 is the third kind)
OK, ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_NOT_FINITE = 0, -1, -2, -3, -4, -5

# The library itself never reads the environment (include/swe2d.h, swe2d_set_option).  As a convenience of THIS binding the variables
# below are read once per handle, right after swe2d_create (Swe2dDevice.__init__), and handed over as options: A/B runs and the parity
# tests that force every kernel variant in turn set them around the construction of a device.  name -> (option, conversion)
OPTION_ENV = {
    'THETIS_AMD_FUSE12': (OPT_FUSED_STAGES, int),
    'THETIS_AMD_FLOW': (OPT_FLOW, int),
    'THETIS_AMD_FLOW_WD': (OPT_FLOW_WD, int),
    'THETIS_AMD_BND_INLINE': (OPT_BND_INLINE, int),
    'THETIS_AMD_LDSX': (OPT_LDSX, int),
    'THETIS_AMD_ALTERNATE': (OPT_ALTERNATE, int),
    'THETIS_AMD_COMPACT_IDX': (OPT_COMPACT_IDX, int),
    'THETIS_AMD_NO_VISC_FUSION': (OPT_VISC_FUSION, lambda v: 0),
    'THETIS_AMD_WALL_FAST': (OPT_WALL_FAST, int),
    'THETIS_AMD_FLOW_POLL': (OPT_FLOW_POLL, int),
    'THETIS_AMD_FLOW_CAPACITY': (OPT_FLOW_CAPACITY, int),
    'THETIS_AMD_FLOW_TIMEOUT_S': (OPT_FLOW_TIMEOUT_MS, lambda v: max(1, int(round(1e3*float(v))))),
    'THETIS_AMD_P2P_TIMEOUT_S': (OPT_P2P_TIMEOUT_MS, lambda v: max(1, int(round(1e3*float(v))))),
    'THETIS_AMD_P2P_ZONE': (OPT_P2P_ZONE, lambda v: {'uncached': 1, 'finegrained': 2, 'device': 3}[v]),
    'THETIS_AMD_ROCTX': (OPT_ROCTX, int),
}


def options_from_environment():
    """[(option, value)] for the variables of OPTION_ENV that are set.  A value the conversion does not accept is reported with a
    warning and left out: the option keeps the library's own rule (an A/B switch must not stop every device constructor)."""
    out = []
    for name, (opt, conv) in OPTION_ENV.items():
        v = os.environ.get(name)
        if v is not None and v != '':
            try:
                out.append((opt, int(conv(v))))
            except (ValueError, KeyError, TypeError) as e:
                warnings.warn('{}={!r} is not a valid value ({}: {}): the library\'s own rule applies'.format(name, v, type(e).__name__, e))
    return out


_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_bp = ctypes.POINTER(ctypes.c_int8)


class Swe2dMesh(ctypes.Structure):
    _fields_ = [('n_cells', ctypes.c_int32), ('n_owned', ctypes.c_int32), ('n_vertices', ctypes.c_int32),
                ('nodes_per_cell', ctypes.c_int32), ('cell_vertices', _ip), ('vertex_xy', _dp),
                ('cell_neighbours', _ip), ('cell_neighbour_facets', _bp), ('bathymetry', _dp),
                ('boundary_len', _dp)]


class Swe2dParams(ctypes.Structure):
    _fields_ = [('g_grav', ctypes.c_double), ('dt', ctypes.c_double),
                ('use_nonlinear_equations', ctypes.c_int32), ('use_lax_friedrichs_velocity', ctypes.c_int32),
                ('lax_friedrichs_velocity_scaling_factor', ctypes.c_double), ('device_id', ctypes.c_int32)]


class TurbineParams(ctypes.Structure):
    """include/swe2d.h swe2d_turbine_params"""
    _fields_ = [('thrust_area_const', ctypes.c_double), ('support_area', ctypes.c_double), ('rotor_area', ctypes.c_double),
                ('projected_diameter', ctypes.c_double), ('power_const', ctypes.c_double), ('rho0', ctypes.c_double),
                ('upwind_correction', ctypes.c_int32), ('n_table', ctypes.c_int32),
                ('speeds', ctypes.c_double*MAX_THRUST_TABLE), ('thrust', ctypes.c_double*MAX_THRUST_TABLE),
                ('power', ctypes.c_double*MAX_THRUST_TABLE)]


class SedimentParams(ctypes.Structure):
    """include/swe2d.h swe2d_sediment_params"""
    _fields_ = [('ws', ctypes.c_double), ('dstar', ctypes.c_double), ('taucr', ctypes.c_double), ('a', ctypes.c_double),
                ('ksp', ctypes.c_double), ('ks', ctypes.c_double), ('rho0', ctypes.c_double), ('kappa', ctypes.c_double),
                ('fac', ctypes.c_double), ('erosion_factor', ctypes.c_double), ('min_depth', ctypes.c_double),
                ('conservative', ctypes.c_int32), ('solve_exner', ctypes.c_int32)]


class BedloadParams(ctypes.Structure):
    """include/swe2d.h swe2d_bedload_params"""
    _fields_ = [('beta', ctypes.c_double), ('surbeta2', ctypes.c_double), ('alpha_secc', ctypes.c_double), ('thetacr', ctypes.c_double),
                ('shields_den', ctypes.c_double), ('qb_scale', ctypes.c_double), ('ks', ctypes.c_double), ('ksp', ctypes.c_double),
                ('kappa', ctypes.c_double), ('rho0', ctypes.c_double), ('fac', ctypes.c_double), ('min_depth', ctypes.c_double),
                ('use_slope_mag_correction', ctypes.c_int32), ('use_angle_correction', ctypes.c_int32),
                ('use_secondary_current', ctypes.c_int32), ('solve_exner', ctypes.c_int32), ('open_markers', ctypes.c_uint32), ('fuse_with_sediment', ctypes.c_int32)]


class SlideParams(ctypes.Structure):
    """include/swe2d.h swe2d_slide_params"""
    _fields_ = [('tanphi', ctypes.c_double), ('length_scale', ctypes.c_double), ('porosity', ctypes.c_double), ('morfac', ctypes.c_double),
                ('fac', ctypes.c_double), ('min_depth', ctypes.c_double), ('solve_exner', ctypes.c_int32)]


# every symbol include/swe2d.h declares: name -> (restype, argtypes)
_H = ctypes.c_void_p
SYMBOLS = {
    'swe2d_abi_version': (ctypes.c_int, []),
    'swe2d_connectivity_info': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_fused_pair_info': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_fused_triple_info': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_fused_set_order': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_solve_step_cells': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_fused_step_info': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_fused_set_triple_tiles': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]),
    'swe2d_solve_stage_pair_cells': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_device_count': (ctypes.c_int, []),
    'swe2d_ssprk33_coefficients': (None, [_dp, _dp, _dp]),
    'swe2d_create': (ctypes.c_int, [ctypes.POINTER(Swe2dMesh), ctypes.POINTER(Swe2dParams), ctypes.POINTER(_H)]),
    'swe2d_destroy': (None, [_H]),
    'swe2d_last_error': (ctypes.c_char_p, [_H]),
    'swe2d_set_state': (ctypes.c_int, [_H, _dp, _dp]),
    'swe2d_get_state': (ctypes.c_int, [_H, _dp, _dp]),
    'swe2d_get_stage_state': (ctypes.c_int, [_H, ctypes.c_int, _dp, _dp]),
    'swe2d_state_snapshot': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_state_snapshot_slot': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_set_option': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_get_option': (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    'swe2d_set_dt': (ctypes.c_int, [_H, ctypes.c_double]),
    'swe2d_set_bc': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, _dp]),
    'swe2d_set_bc_field': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, _dp]),
    'swe2d_set_bc_facets': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32, _ip, _ip, _dp]),
    'swe2d_set_boundary_drag': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_double]),
    'swe2d_set_field': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_set_field_vertex': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_set_scalar': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_double]),
    'swe2d_set_wetting_and_drying': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_set_viscosity': (ctypes.c_int, [_H, ctypes.c_int, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int]),
    'swe2d_advance': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_solve_stage': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_advance_timed': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float)]),
    'swe2d_synchronize': (ctypes.c_int, [_H]),
    'swe2d_tendency': (ctypes.c_int, [_H, _dp, _dp]),
    'swe2d_diagnostics': (ctypes.c_int, [_H, _dp]),
    'swe2d_diagnostics_limbs': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64), _dp]),
    'swe2d_sum_limbs_to_double': (ctypes.c_double, [ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_tracer_diagnostics_limbs': (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), _dp]),
    'swe2d_set_general_quadrilaterals': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_tracer_add': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int)]),
    'swe2d_tracer_set_options': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    'swe2d_tracer_set_state': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_tracer_get_state': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_tracer_set_bc': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    'swe2d_tracer_set_bc_velocity': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]),
    'swe2d_tracer_set_bc_velocity_facets': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int32,
                                                            _ip, _ip, _dp]),
    'swe2d_tracer_set_bc_field': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, _dp]),
    'swe2d_tracer_set_bc_facets': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32, _ip, _ip, _dp]),
    'swe2d_tracer_set_source': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_tracer_solve_stage_cells': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_tracer_swap_buffers': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_tracer_limit_cells': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32]),
    'swe2d_tracer_halo_pack': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'swe2d_tracer_halo_unpack': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'swe2d_advance_forward_euler': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_tracer_forward_euler': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_tracer_set_conservative': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_tracer_set_diffusivity': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_double, ctypes.c_double]),
    'swe2d_tracer_set_diffusion_bc': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]),
    'swe2d_tracer_solve_stage': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_tracer_tendency': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_limiter_setup': (ctypes.c_int, [_H, ctypes.c_int32, _ip]),
    'swe2d_tracer_limit': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_tracer_diagnostics': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_advance_coupled': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'swe2d_debug_calibration_copy': (ctypes.c_int, [_H, ctypes.c_int]),
    'swe2d_debug_live_device_memory': (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64)]),
    'swe2d_halo_setup': (ctypes.c_int, [_H, ctypes.c_int32, _ip, ctypes.c_int32, _ip]),
    'swe2d_halo_pack': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_void_p]),
    'swe2d_halo_unpack': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_void_p]),
    'swe2d_p2p_create': (ctypes.c_int, [_H, ctypes.c_int32, _ip]),
    'swe2d_p2p_export': (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), _ip]),
    'swe2d_p2p_open': (ctypes.c_int, [_H, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    'swe2d_p2p_connect': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), _ip, _ip, _ip, _ip, _ip,
                                          ctypes.c_int32]),
    'swe2d_p2p_push': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_p2p_wait_unpack': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_p2p_push_multi': (ctypes.c_int, [_H, ctypes.c_int, _ip, _ip]),
    'swe2d_p2p_wait_unpack_multi': (ctypes.c_int, [_H, ctypes.c_int, _ip, _ip]),
    'swe2d_p2p_status': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), _ip]),
    'swe2d_solve_stage_cells': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_forward_euler_cells': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_swap_state_buffers': (ctypes.c_int, [_H]),
    'swe2d_solve_flow': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_flow_supported': (ctypes.c_int, [_H]),
    'swe2d_flow_prepare_exchange': (ctypes.c_int, [_H]),
    'swe2d_flow_unpack_pending': (ctypes.c_int, [_H]),
    'swe2d_solve_flow_exchange': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_flow_set_order': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_flow_status': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int32)]),
    'swe2d_debug_flow_poke': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_debug_flow_delay': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_debug_flow_tear': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_set_stream': (ctypes.c_int, [_H, ctypes.c_void_p]),
    'swe2d_set_exchange_stream': (ctypes.c_int, [_H, ctypes.c_void_p]),
    'swe2d_probe_create': (ctypes.c_int, [_H, ctypes.c_int32, _ip, _dp, ctypes.c_int32, _ip, ctypes.c_int32, _ip]),
    'swe2d_probe_width': (ctypes.c_int, [_H, ctypes.c_int32, _ip, _ip, _ip]),
    'swe2d_probe_append': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_probe_read': (ctypes.c_int, [_H, ctypes.c_int32, _dp, _ip]),
    'swe2d_probe_eval': (ctypes.c_int, [_H, ctypes.c_int32, _dp]),
    'swe2d_probe_destroy': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_turbine_farm_set': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.POINTER(TurbineParams), _dp]),
    'swe2d_turbine_farm_clear': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_turbine_power': (ctypes.c_int, [_H, _dp]),
    'swe2d_turbine_power_limbs': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_turbine_rows_reserve': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_turbine_rows_append': (ctypes.c_int, [_H]),
    'swe2d_turbine_rows_read': (ctypes.c_int, [_H, _dp, _ip]),
    'swe2d_dfarm_set': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.POINTER(TurbineParams), ctypes.c_int32, _dp,
                                       ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, _dp, _dp]),
    'swe2d_dfarm_density_read': (ctypes.c_int, [_H, ctypes.c_int32, _ip, _ip, _ip, _dp]),
    'swe2d_dfarm_turbine_power': (ctypes.c_int, [_H, ctypes.c_int32, _dp]),
    'swe2d_tide_set': (ctypes.c_int, [_H, ctypes.c_int32, _ip, _ip, ctypes.c_int32, _dp, _dp, _dp, _dp]),
    'swe2d_tide_clear': (ctypes.c_int, [_H]),
    'swe2d_tide_clock': (ctypes.c_int, [_H, ctypes.c_double, ctypes.c_int64]),
    'swe2d_tide_eval': (ctypes.c_int, [_H, ctypes.c_double]),
    'swe2d_tide_read': (ctypes.c_int, [_H, _dp]),
    'swe2d_atm_set': (ctypes.c_int, [_H, ctypes.c_int32, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32]),
    'swe2d_atm_clear': (ctypes.c_int, [_H]),
    'swe2d_atm_eval': (ctypes.c_int, [_H, ctypes.c_double]),
    'swe2d_atm_read': (ctypes.c_int, [_H, _dp, _dp]),
    'swe2d_stats_create': (ctypes.c_int, [_H, ctypes.c_int32, _ip]),
    'swe2d_stats_append': (ctypes.c_int, [_H, ctypes.c_int32, _dp]),
    'swe2d_stats_read': (ctypes.c_int, [_H, ctypes.c_int32, _dp, ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_stats_reset': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_stats_destroy': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_particles_create': (ctypes.c_int, [_H, ctypes.c_int32, _dp, _ip, ctypes.c_int32, _ip]),
    'swe2d_particles_advance': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, _ip]),
    'swe2d_particles_record': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_particles_read': (ctypes.c_int, [_H, ctypes.c_int32, _dp, _ip, _ip, _ip, _ip]),
    'swe2d_particles_read_rows': (ctypes.c_int, [_H, ctypes.c_int32, _dp, _ip]),
    'swe2d_particles_destroy': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_particles_set_diffusivity': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_uint64]),
    'swe2d_particles_set_release_times': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_double]),
    'swe2d_particles_advance_at': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, _ip]),
    'swe2d_particles_cell_counts': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_uint32, _ip]),
    'swe2d_tracer_set_reaction': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32, _ip, ctypes.c_int32, _dp, ctypes.c_int32, _dp, _dp]),
    'swe2d_tracer_set_reaction_constants': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int32, _dp]),
    'swe2d_reaction_set_field': (ctypes.c_int, [_H, ctypes.c_int32, _dp]),
    'swe2d_tracer_get_source': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
    'swe2d_tracer_get_buffer': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int, _dp]),
    'swe2d_sediment_set': (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(SedimentParams)]),
    'swe2d_sediment_set_equilibrium_bc': (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_int]),
    'swe2d_sediment_update': (ctypes.c_int, [_H]),
    'swe2d_sediment_read': (ctypes.c_int, [_H, _dp, _dp, _dp]),
    'swe2d_sediment_read_bc': (ctypes.c_int, [_H, _dp]),
    'swe2d_sediment_clear': (ctypes.c_int, [_H]),
    'swe2d_exner_step': (ctypes.c_int, [_H]),
    'swe2d_exner_skipped': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_bedload_set': (ctypes.c_int, [_H, ctypes.POINTER(BedloadParams)]),
    'swe2d_bedload_update': (ctypes.c_int, [_H]),
    'swe2d_bedload_read': (ctypes.c_int, [_H, _dp, _dp, _dp]),
    'swe2d_bedload_clear': (ctypes.c_int, [_H]),
    'swe2d_slide_set': (ctypes.c_int, [_H, ctypes.POINTER(SlideParams), _dp]),
    'swe2d_slide_update': (ctypes.c_int, [_H]),
    'swe2d_slide_read': (ctypes.c_int, [_H, _dp, _dp, _dp]),
    'swe2d_slide_max_angle': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_double)]),
    'swe2d_slide_flagged': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_slide_clear': (ctypes.c_int, [_H]),
    'swe2d_get_bathymetry': (ctypes.c_int, [_H, _dp]),
    'swe2d_set_bathymetry': (ctypes.c_int, [_H, _dp]),
    'swe2d_sections_set': (ctypes.c_int, [_H, ctypes.c_int32, ctypes.c_int32, _ip, _ip, _dp, _dp, ctypes.c_int32, _ip]),
    'swe2d_sections_clear': (ctypes.c_int, [_H]),
    'swe2d_sections_eval_limbs': (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_sections_eval': (ctypes.c_int, [_H, _dp, ctypes.POINTER(ctypes.c_int64)]),
    'swe2d_sections_rows_reserve': (ctypes.c_int, [_H, ctypes.c_int32]),
    'swe2d_sections_rows_append': (ctypes.c_int, [_H]),
    'swe2d_sections_rows_read': (ctypes.c_int, [_H, _dp, ctypes.POINTER(ctypes.c_int64), _ip]),
    'swe2d_smag_set': (ctypes.c_int, [_H, ctypes.c_double, _dp, ctypes.c_double, ctypes.c_double, _ip, _ip]),
    'swe2d_smag_clear': (ctypes.c_int, [_H]),
    'swe2d_smag_update': (ctypes.c_int, [_H]),
    'swe2d_smag_read': (ctypes.c_int, [_H, ctypes.c_int, _dp]),
}

_lib = None


class Swe2dError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('swe2d error {:d}: {:s}'.format(code, msg))
        self.code = code


def load():
    """Load libswe2d_hip.so (built by ``thetis_amd._build.build`` / ``__graft_entry__.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('HIP extension {:} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                          '(there is no CPU fallback)'.format(LIB_PATH))
    # PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process do not see each other's devices.
    # Import torch first (when present) so that the extension binds to the runtime torch uses for RCCL / streams.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)     # AttributeError if the library does not export a declared symbol
        except AttributeError:
            if os.environ.get('THETIS_AMD_LIB'):
                continue                # kernel A/B experiments against older builds (tools/kbench.py)
            raise
        fn.restype = restype
        fn.argtypes = argtypes
    if not os.environ.get('THETIS_AMD_LIB') and lib.swe2d_abi_version() != ABI_VERSION:
        raise ImportError('{:} implements ABI version {:d}, this package binds version {:d}: rebuild it '
                          '(python -c "import __graft_entry__ as g; g.build()")'.format(LIB_PATH, lib.swe2d_abi_version(),
                                                                                          ABI_VERSION))
    _lib = lib
    return lib


def check(rc, handle=None):
    if rc != OK:
        msg = load().swe2d_last_error(handle)
        raise Swe2dError(rc, msg.decode() if msg else '')
