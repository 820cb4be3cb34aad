"""Random option combinations of the shallow-water stage, shared by the randomised GPU tests (plain module, no GPU needed).

``random_config`` draws what tests/test_gpu_fuzz.py always drew - same rng calls in the same order, so its seeds test what they
tested before.  ``tiles_only=True`` is a second stream (drawn from seeds of its own by tests/test_gpu_fuzz_paths.py) restricted to
what the tile kernels of csrc/swe2d_fuse.h cover; ``perturb`` gives a second set of values for the same kinds: forcing that changes
between steps.  ``path_case`` / ``quad_path_case`` / ``partition_case`` hold everything a seed of the path fuzz decides, so that
tests/test_fuzz_cases.py can count on the CPU what the GPU file covers."""
import hashlib

import numpy as np

from helpers import channel_case, delaunay_case, quad_case
from thetis_amd import _lib

# seed ranges of tests/test_gpu_fuzz_paths.py (rng streams: 20000 + seed, 30000 + seed, 40000 + seed)
TRI_SEEDS = range(96)
QUAD_SEEDS = range(48)
PARTITION_SEEDS = range(16)
PATCHES = [(6, 4), (5, 3), (11, 8)]
REORDERS = ['auto', 'hilbert', None]
KINDS = [None, {'elev': 1}, {'uv': 1}, {'un': 1}, {'flux': 1}, {'elev': 1, 'uv': 1}, {'elev': 1, 'un': 1}, {'elev': 1, 'flux': 1}]
# the smallest quad_case for which fused_pair_info() reports 3 tiles (tiles of at most 192 interior cells + a ring of at most 64:
# 24 x 16 = 384 cells are two full tiles; asserted in tests/test_gpu_fuzz_paths.py)
QUAD_NX, QUAD_NY = 25, 16

# oracle keyword of every source field the device takes through set_field
FIELD_KEYS = {_lib.FIELD_CORIOLIS: 'coriolis', _lib.FIELD_ATMOSPHERIC_PRESSURE: 'atmospheric_pressure',
              _lib.FIELD_MOMENTUM_SOURCE: 'momentum_source', _lib.FIELD_VOLUME_SOURCE: 'volume_source',
              _lib.FIELD_WIND_STRESS: 'wind_stress', _lib.FIELD_LINEAR_DRAG: 'linear_drag_coefficient',
              _lib.FIELD_MANNING_DRAG: 'manning_drag_coefficient', _lib.FIELD_QUADRATIC_DRAG: 'quadratic_drag_coefficient'}
SOURCE_FIELDS = ('coriolis', 'atmospheric_pressure', 'momentum_source', 'volume_source', 'wind_stress')
DRAG_SCALARS = {_lib.SCALAR_LINEAR_DRAG: 'linear_drag_coefficient', _lib.SCALAR_QUADRATIC_DRAG: 'quadratic_drag_coefficient',
                _lib.SCALAR_MANNING_DRAG: 'manning_drag_coefficient', _lib.SCALAR_NIKURADSE: 'nikuradse_bed_roughness'}


def random_config(rng, mesh, quad, tiles_only=False):
    """(oracle kwargs, device calls (name, args[, kwargs]), boundary dicts by marker, wetting-drying?)

    ``tiles_only``: nothing the tile kernels decline (csrc/swe2d_plan.hip step_kernels(): `if (h->wd) k &= ... kFlow : 0u` and
    `if (h->visc) k = 0`) - no wetting-drying, no viscosity; and one draw in five carries no source term at all, so that the
    instances without source terms meet boundaries of every kind (has_sources() of csrc/swe2d_handle.h picks the instance, and
    boundary data and boundary drag are not part of it)."""
    n, k = mesh.num_cells, mesh.cells.shape[1]
    x, y = mesh.vertex_xy.T
    o, dev_ops = {}, []                       # oracle kwargs, device calls (name, args)
    bare = tiles_only and rng.random() < 0.2
    nonlin = bool(rng.integers(0, 2))
    wd = not tiles_only and nonlin and rng.random() < 0.25
    o['use_nonlinear_equations'] = nonlin
    o['use_lax_friedrichs_velocity'] = bool(rng.integers(0, 2))
    o['lax_friedrichs_velocity_scaling_factor'] = float(rng.choice([1.0, 0.6]))
    if wd:
        o.update(use_wetting_and_drying=True, wetting_and_drying_alpha=0.5 + 0.3*rng.random(), wd_mode='nodal')
        dev_ops.append(('set_wetting_and_drying', (o['wetting_and_drying_alpha'],)))
    if rng.random() < 0.5 and not bare:
        cor = 1e-4*(1 + y/(abs(y).max() + 1.0))
        o['coriolis'] = cor
        dev_ops.append(('set_field', (_lib.FIELD_CORIOLIS, cor[mesh.cells])))
    if rng.random() < 0.4 and not bare:
        pa = 1e5 + 300*np.sin(x/2e4)
        o['atmospheric_pressure'] = pa
        dev_ops.append(('set_field', (_lib.FIELD_ATMOSPHERIC_PRESSURE, pa[mesh.cells])))
    if rng.random() < 0.4 and not bare:
        ms = 1e-3*rng.normal(size=(n, k, 2))
        o['momentum_source'] = ms
        dev_ops.append(('set_field', (_lib.FIELD_MOMENTUM_SOURCE, ms)))
    if rng.random() < 0.4 and not bare:
        vs = 1e-3*rng.normal(size=(n, k))
        o['volume_source'] = vs
        dev_ops.append(('set_field', (_lib.FIELD_VOLUME_SOURCE, vs)))
    if rng.random() < 0.3 and not bare:
        ws = 0.1*rng.normal(size=(n, k, 2))
        o['wind_stress'] = ws
        dev_ops.append(('set_field', (_lib.FIELD_WIND_STRESS, ws)))
    lin = 1.0 if bare else rng.random()
    if lin < 0.25:
        o['linear_drag_coefficient'] = 1e-3
        dev_ops.append(('set_scalar', (_lib.SCALAR_LINEAR_DRAG, 1e-3)))
    elif lin < 0.45:
        c = 1e-3*(1 + x/(abs(x).max() + 1.0))
        o['linear_drag_coefficient'] = c
        dev_ops.append(('set_field', (_lib.FIELD_LINEAR_DRAG, c[mesh.cells])))
    drag = 0 if bare else rng.integers(0, 7)
    field = 1.0 + 0.5*x/(abs(x).max() + 1.0)
    if drag == 1:
        o['quadratic_drag_coefficient'] = 0.0025
        dev_ops.append(('set_scalar', (_lib.SCALAR_QUADRATIC_DRAG, 0.0025)))
    elif drag == 2:
        o['manning_drag_coefficient'] = 0.02
        dev_ops.append(('set_scalar', (_lib.SCALAR_MANNING_DRAG, 0.02)))
    elif drag == 3:
        o['nikuradse_bed_roughness'] = 0.05
        dev_ops.append(('set_scalar', (_lib.SCALAR_NIKURADSE, 0.05)))
    elif drag == 4:
        o['manning_drag_coefficient'] = 0.02*field
        dev_ops.append(('set_field', (_lib.FIELD_MANNING_DRAG, (0.02*field)[mesh.cells])))
    elif drag == 5:
        o['quadratic_drag_coefficient'] = 0.0025*field
        dev_ops.append(('set_field', (_lib.FIELD_QUADRATIC_DRAG, (0.0025*field)[mesh.cells])))
    if drag and rng.random() < 0.5:
        o['norm_smoother'] = 0.05
        dev_ops.append(('set_scalar', (_lib.SCALAR_NORM_SMOOTHER, 0.05)))
    visc = None
    if not tiles_only and rng.random() < 0.4:
        nu = 30.0 if rng.random() < 0.5 else 20.0 + 20.0*rng.uniform(size=mesh.num_vertices)
        visc = dict(sipg_factor=float(rng.choice([1.0, 2.0])), use_grad_div_viscosity_term=bool(rng.integers(0, 2)),
                    use_grad_depth_viscosity_term=bool(rng.integers(0, 2)))
        o.update(horizontal_viscosity=nu, **visc)
        dev_ops.append(('set_viscosity', (nu,), visc))
    # boundaries
    bcs = {}
    for marker in (1, 2, 3, 4):
        kind = KINDS[int(rng.integers(0, len(KINDS)))]
        funcs = {}
        for key in (kind or {}):
            funcs[key] = _bc_value(rng, key, rng.random() < 0.4, n, k)
        if rng.random() < 0.2:
            funcs['drag'] = 0.01
        if funcs:
            bcs[marker] = funcs
    o['bnd_conditions'] = bcs
    return o, dev_ops, bcs, wd


def _bc_value(rng, key, as_field, n, k):
    if key == 'elev':
        return 0.1*rng.normal(size=(n, k)) if as_field else 0.1*rng.normal()
    if key == 'uv':
        return 0.2*rng.normal(size=(n, k, 2)) if as_field else tuple(0.2*rng.normal(size=2))
    if key == 'un':
        return 0.2*rng.normal(size=(n, k)) if as_field else 0.2*rng.normal()
    return 2e4*rng.normal(size=(n, k)) if as_field else 2e4*rng.normal()


def perturb(rng, o, dev_ops, bcs):
    """A second set of values for the kinds of (o, dev_ops, bcs): every boundary constant and field drawn again (constants stay
    constants, fields stay fields, the boundary drag changes), one source field and one drag scalar rescaled.  Returns
    (oracle kwargs, the device calls that change, boundary dicts); nothing of the input is modified."""
    o2, ops2, bcs2 = dict(o), [], {}
    for marker, funcs in bcs.items():
        new = {}
        for key, val in funcs.items():
            if key == 'drag':
                new[key] = val*(1.0 + rng.random())
            else:
                shape = np.shape(val)
                as_field = len(shape) >= 2
                new[key] = _bc_value(rng, key, as_field, *(shape[:2] if as_field else (0, 0)))
        bcs2[marker] = new
    o2['bnd_conditions'] = bcs2
    fields = [op for op in dev_ops if op[0] == 'set_field']
    if fields:
        _, (fid, arr) = fields[int(rng.integers(0, len(fields)))]
        fac = 1.25 + 0.5*rng.random()
        o2[FIELD_KEYS[fid]] = fac*np.asarray(o[FIELD_KEYS[fid]])
        ops2.append(('set_field', (fid, fac*np.asarray(arr))))
    scalars = [op for op in dev_ops if op[0] == 'set_scalar' and op[1][0] in DRAG_SCALARS]
    if scalars:
        _, (sid, val) = scalars[int(rng.integers(0, len(scalars)))]
        fac = 1.25 + 0.5*rng.random()
        o2[DRAG_SCALARS[sid]] = fac*val
        ops2.append(('set_scalar', (sid, fac*val)))
    return o2, ops2, bcs2


def has_sources(dev_ops):
    """csrc/swe2d_handle.h has_sources(): a source field or one of the four drag scalars (not the norm smoother, not the boundaries)"""
    return any(op[0] == 'set_field' or (op[0] == 'set_scalar' and op[1][0] in DRAG_SCALARS) for op in dev_ops)


def describe(o):
    return {kk: (vv if np.isscalar(vv) or isinstance(vv, (bool, str)) else type(vv).__name__) for kk, vv in o.items()}


def _digest_update(hs, v):
    if isinstance(v, dict):
        for kk in sorted(v, key=str):
            hs.update(repr(kk).encode())
            _digest_update(hs, v[kk])
    elif isinstance(v, (bool, str)) or v is None:
        hs.update(repr(v).encode())
    else:
        a = np.asarray(v, dtype=np.float64)
        hs.update(repr(a.shape).encode())
        hs.update(np.ascontiguousarray(a).tobytes())


def options_digest(configs):
    """sha256 over the option dictionaries (keys, shapes and the bytes of every value as float64) of an iterable of draws"""
    hs = hashlib.sha256()
    for o in configs:
        _digest_update(hs, o)
    return hs.hexdigest()


def legacy_case(seed):
    """mesh and draw of tests/test_gpu_fuzz.py::test_random_option_combinations_match_oracle"""
    quad = seed % 3 == 2
    if quad:
        mesh, bath, uv, eta = quad_case(nx=7, ny=5, skew=0.25, seed=seed)
    else:
        mesh, bath, uv, eta = channel_case(nx=7, ny=5, seed=seed)
    o, dev_ops, bcs, wd = random_config(np.random.default_rng(1000 + seed), mesh, quad)
    return mesh, bath, uv, eta, o, dev_ops, bcs, wd


# ---- what a seed of tests/test_gpu_fuzz_paths.py decides ------------------------------------------------------------------------------
_MESHES = {}


def _mesh_of(kind, seed):
    """meshes are shared between seeds (the state is drawn per seed): 'channel' 24 x 16 = 768 cells, 4 tiles cut from the numbering
    and 16 under patches of 6 x 4; 'ragged' 29 x 13 = 754 cells; 'delaunay': ~400 random points, one of four triangulations"""
    key = (kind, seed % 4 if kind == 'delaunay' else 0)
    if key not in _MESHES:
        if kind == 'channel':
            mesh, bath = channel_case(nx=24, ny=16, lx=100e3, ly=50e3)[:2]
        elif kind == 'ragged':
            mesh, bath = channel_case(nx=29, ny=13, lx=100e3, ly=50e3)[:2]
        else:
            mesh, bath = delaunay_case(n_points=400, seed=key[1])[:2]
        _MESHES[key] = (mesh, bath)
    return _MESHES[key]


TRI_MESH_KINDS = ('channel', 'ragged', 'delaunay')
QUAD_MESH_KINDS = ('skew', 'warp', 'rect')


def _state(rng, mesh, amp_u, amp_eta):
    n, k = mesh.num_cells, mesh.cells.shape[1]
    uv = amp_u*rng.normal(size=(n, k, 2))
    eta = np.abs(amp_eta*rng.normal(size=(n, k)))          # keep the depth positive for the drag terms
    return uv, eta


def path_case(seed, stream=20000):
    """triangles: dict with mesh kind, mesh, bathymetry, state, dt, reorder, patch size (structured meshes: else None), the
    restricted draw (o, dev_ops, bcs) and its perturbation (o2, ops2, bcs2)"""
    rng = np.random.default_rng(stream + seed)
    kind = TRI_MESH_KINDS[seed % 3]
    mesh, bath = _mesh_of(kind, seed)
    c = dict(seed=seed, kind=kind, mesh=mesh, bath=bath, quad=False)
    c['reorder'] = REORDERS[int(rng.integers(0, 3))]
    patch = PATCHES[int(rng.integers(0, 3))]
    c['patch'] = patch if kind != 'delaunay' else None
    c['uv'], c['eta'] = _state(rng, mesh, 0.3, 0.3)
    c['dt'] = 0.5 if kind != 'delaunay' else 0.05
    c['o'], c['dev_ops'], c['bcs'], wd = random_config(rng, mesh, False, tiles_only=True)
    assert not wd
    c['o2'], c['ops2'], c['bcs2'] = perturb(rng, c['o'], c['dev_ops'], c['bcs'])
    return c


def quad_path_case(seed):
    """quadrilaterals, QUAD_NX x QUAD_NY cells: skewed parallelograms / general cells / rectangles by seed % 3"""
    rng = np.random.default_rng(30000 + seed)
    kind = QUAD_MESH_KINDS[seed % 3]
    key = ('quad', kind)
    if key not in _MESHES:
        kw = dict(skew=0.25) if kind == 'skew' else (dict(warp=0.2) if kind == 'warp' else {})
        _MESHES[key] = quad_case(nx=QUAD_NX, ny=QUAD_NY, seed=0, **kw)[:2]
    mesh, bath = _MESHES[key]
    c = dict(seed=seed, kind=kind, mesh=mesh, bath=bath, quad=True, patch=None)
    c['reorder'] = REORDERS[int(rng.integers(0, 3))]
    c['uv'], c['eta'] = _state(rng, mesh, 0.3, 0.3)
    c['dt'] = 0.5
    c['o'], c['dev_ops'], c['bcs'], wd = random_config(rng, mesh, True, tiles_only=True)
    assert not wd
    c['o2'], c['ops2'], c['bcs2'] = perturb(rng, c['o'], c['dev_ops'], c['bcs'])
    return c


def partition_case(seed):
    """the triangle case of stream 40000 + seed, and where in the last / second-last tile (as a fraction) cell_end falls"""
    c = path_case(seed, stream=40000)
    rng = np.random.default_rng(45000 + seed)
    c['tile_from_end'] = int(rng.integers(1, 3))            # 1: the last tile, 2: the one before
    c['frac'] = float(rng.uniform(0.05, 0.95))
    return c


def apply_config(dev, dev_ops, bcs):
    for op in dev_ops:
        getattr(dev, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
    for marker, funcs in bcs.items():
        dev.set_bc(marker, funcs)
