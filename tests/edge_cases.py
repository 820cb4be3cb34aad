"""Launch shapes at the edges of a wave, a workgroup and a tile, and cell ranges cut at those edges (plain module, no GPU needed).

The stage kernels run 64 cells per workgroup (SWE_BLOCK), the helper kernels 256 lanes, a tile holds 192 interior cells or 256
lanes.  ``TRI_SIZES`` / ``QUAD_SIZES`` are meshes whose cell counts sit at 0 and +-1 (triangle counts are even: +-2) of 64, 128, 192,
256 and 512, strips one cell wide and the one-cell mesh among them; every cell is the same 2 km square (cut in two).  ``case`` holds one
fixed set of configurations on them, ``tracer_setup`` one tracer; ``split_ranges`` and the drivers below launch a stage range by range
on whatever stands in for a device (``thetis_amd.device.Swe2dDevice``, tests/cpu_device.py), so that tests/test_edge_cases.py proves
the logic of tests/test_gpu_launch_edges.py with the reference alone."""
import numpy as np

from helpers import channel_case, quad_case
from thetis_amd import _lib

# (nx, ny): 2*nx*ny triangles
TRI_SIZES = [(1, 1), (3, 1), (31, 1), (8, 4), (11, 3), (9, 7), (8, 8), (13, 5), (19, 5), (12, 8), (97, 1), (127, 1), (16, 8), (43, 3),
             (17, 15), (16, 16), (257, 1)]
# (nx, ny): nx*ny quadrilaterals, each as parallelograms and as general cells
QUAD_SIZES = [(1, 1), (2, 1), (9, 7), (8, 8), (13, 5), (127, 1), (16, 8), (43, 3), (191, 1), (16, 12), (193, 1), (17, 15), (16, 16),
              (257, 1)]
QUAD_GEOMETRIES = {'skew': dict(skew=0.25), 'warp': dict(warp=0.2)}
KINDS = ('tri',) + tuple(QUAD_GEOMETRIES)
CONFIGS = ('a', 'b', 'c', 'd')
VISC_MAX_CELLS = 258                          # configuration (d) runs on the sizes up to 258 triangles / 257 quadrilaterals
CELL = 2e3                                    # edge of the square every cell is (half of)
# wetting-drying: the shift of the bathymetry that leaves the mesh partly dry, by (kind, nx, ny) where 12.0 does not
WD_SHIFT = {}
SPLIT_FROM = 130                              # the smallest mesh split_points() cuts


def num_cells(kind, nx, ny):
    return (2 if kind == 'tri' else 1)*nx*ny


def sizes(kind):
    return TRI_SIZES if kind == 'tri' else QUAD_SIZES


def size_cases():
    """every (kind, nx, ny, configuration) of the size tests, in a fixed order"""
    out = []
    for kind in KINDS:
        for nx, ny in sizes(kind):
            for cfg in CONFIGS:
                if cfg != 'd' or num_cells(kind, nx, ny) <= VISC_MAX_CELLS:
                    out.append((kind, nx, ny, cfg))
    return out


def tracer_cases():
    return [(kind, nx, ny) for kind in KINDS for nx, ny in sizes(kind)]


def case_id(c):
    return '{}-{}x{}'.format(*c[:3]) + ('-' + c[3] if len(c) > 3 else '')


_MESHES = {}


def mesh_case(kind, nx, ny):
    """(mesh, bathymetry, uv, eta) as helpers.channel_case / quad_case draw them, lx = 2 km * nx, ly = 2 km * ny"""
    key = (kind, nx, ny)
    if key not in _MESHES:
        seed = 31*nx + ny
        if kind == 'tri':
            _MESHES[key] = channel_case(nx=nx, ny=ny, lx=CELL*nx, ly=CELL*ny, seed=seed)
        else:
            _MESHES[key] = quad_case(nx=nx, ny=ny, lx=CELL*nx, ly=CELL*ny, seed=seed, **QUAD_GEOMETRIES[kind])
    return _MESHES[key]


def flow_config(mesh, cfg, seed=0):
    """(oracle kwargs, device calls (name, args[, kwargs]), boundary dicts by marker, wetting-drying?) of configuration ``cfg``:
    a  nonlinear, Lax-Friedrichs, constant elev / uv / un / flux on markers 1-4, a Coriolis field, Manning 0.02 with norm_smoother 0.05
    b  linear, no Lax-Friedrichs, walls everywhere, no source term (the instance the three-stage kernel takes by itself)
    c  wetting-drying (nonlinear, alpha 0.6) with Manning
    d  a + viscosity: nu a vertex field, sipg_factor 2.0, grad-div and grad-depth terms"""
    o = dict(use_nonlinear_equations=cfg != 'b', use_lax_friedrichs_velocity=cfg != 'b', lax_friedrichs_velocity_scaling_factor=1.0)
    dev_ops, bcs = [], {}
    if cfg in ('a', 'd'):
        y = mesh.vertex_xy[:, 1]
        cor = 1e-4*(1 + y/(abs(y).max() + 1.0))
        o.update(coriolis=cor, manning_drag_coefficient=0.02, norm_smoother=0.05)
        dev_ops += [('set_field', (_lib.FIELD_CORIOLIS, cor[mesh.cells])), ('set_scalar', (_lib.SCALAR_MANNING_DRAG, 0.02)),
                    ('set_scalar', (_lib.SCALAR_NORM_SMOOTHER, 0.05))]
        bcs = {1: {'elev': 0.1}, 2: {'uv': (0.2, -0.1)}, 3: {'un': 0.15}, 4: {'flux': 4.0*mesh.boundary_len[4]}}
    if cfg == 'c':
        o.update(use_wetting_and_drying=True, wetting_and_drying_alpha=0.6, wd_mode='nodal', manning_drag_coefficient=0.02)
        dev_ops += [('set_wetting_and_drying', (0.6,)), ('set_scalar', (_lib.SCALAR_MANNING_DRAG, 0.02))]
    if cfg == 'd':
        add_viscosity(mesh, o, dev_ops, seed)
    o['bnd_conditions'] = bcs
    return o, dev_ops, bcs, cfg == 'c'


def add_viscosity(mesh, o, dev_ops, seed=0):
    nu = 20.0 + 20.0*np.random.default_rng(7000 + seed).uniform(size=mesh.num_vertices)
    visc = dict(sipg_factor=2.0, use_grad_div_viscosity_term=True, use_grad_depth_viscosity_term=True)
    o.update(horizontal_viscosity=nu, **visc)
    dev_ops.append(('set_viscosity', (nu,), visc))


def case(kind, nx, ny, cfg):
    """everything a size test needs: mesh, bathymetry, state, dt and the configuration"""
    mesh, bath, uv, eta = mesh_case(kind, nx, ny)
    o, dev_ops, bcs, wd = flow_config(mesh, cfg, seed=31*nx + ny)
    if wd:
        bath = bath - WD_SHIFT.get((kind, nx, ny), 12.0)         # partly dry
    else:
        eta = np.abs(eta)                                        # keep the depth positive for the drag terms
    return dict(kind=kind, nx=nx, ny=ny, cfg=cfg, quad=kind != 'tri', mesh=mesh, bath=bath, uv=uv, eta=eta, dt=0.5 if wd else 2.0,
                o=o, dev_ops=dev_ops, bcs=bcs, wd=wd)


def dry_share(c):
    """share of the nodes whose still-water depth h + eta is negative"""
    return float(((c['bath'][c['mesh'].cells] + c['eta']) < 0.0).mean())


def oracle(c):
    from helpers import make_oracle, make_oracle_generic
    return (make_oracle_generic if c['quad'] else make_oracle)(c['mesh'], c['bath'], **c['o'])


def make_device(c, device_cls, reorder='auto'):
    o = c['o']
    dev = device_cls(c['mesh'], c['bath'], c['dt'], use_nonlinear_equations=o['use_nonlinear_equations'],
                     use_lax_friedrichs_velocity=o['use_lax_friedrichs_velocity'],
                     lax_friedrichs_velocity_scaling_factor=o['lax_friedrichs_velocity_scaling_factor'],
                     boundary_len=c['mesh'].boundary_len, reorder=reorder)
    apply_config(dev, c['dev_ops'], c['bcs'])
    return dev


def apply_config(dev, dev_ops, bcs):
    for op in dev_ops:
        getattr(dev, op[0])(*op[1], **(op[2] if len(op) > 2 else {}))
    for marker, funcs in bcs.items():
        dev.set_bc(marker, funcs)


# ---- the tracer ---------------------------------------------------------------------------------------------------------------------
def tracer_setup(mesh, seed=0, plain=False):
    """(initial values, oracle keywords, device calls (name, args after the tracer id)): conservative form, Lax-Friedrichs, a source, a
    diffusivity field, 'value' on marker 1 and 'diff_flux' on marker 2.  ``plain``: what tests/cpu_device.py covers of it
    (non-conservative, no diffusion)."""
    rng = np.random.default_rng(9000 + seed)
    n, k = mesh.num_cells, mesh.cells.shape[1]
    T = 3.0 + rng.normal(size=(n, k))
    src = 1e-3*rng.normal(size=(n, k))
    mu = 15.0 + 10.0*rng.uniform(size=mesh.num_vertices)
    kw = dict(conservative=not plain, use_lax_friedrichs_tracer=True, lax_friedrichs_tracer_scaling_factor=1.0,
              tracer_advective_velocity_factor=1.0, source=src, bnd_conditions={1: {'value': 1.5}})
    ops = [('tracer_set_conservative', (not plain,)), ('tracer_set_source', (src,)), ('tracer_set_bc', (1, 1.5))]
    if not plain:
        kw.update(diffusivity=mu, sipg_factor_tracer=1.7)
        kw['bnd_conditions'][2] = {'diff_flux': 0.03}
        # kinds of swe2d_tracer_set_diffusion_bc: 1 a prescribed diffusive flux, 2 a constant boundary value
        ops += [('tracer_set_diffusivity', (mu, 1.7)), ('tracer_set_diffusion_bc', (1, 2, 0.0)), ('tracer_set_diffusion_bc', (2, 1, 0.03))]
    return T, kw, ops


def add_tracer(dev, ops):
    tid = dev.add_tracer()
    dev.tracer_set_options(True, 1.0, 1.0)
    for name, args in ops:
        getattr(dev, name)(tid, *args)
    return tid


def tracer_buffer(dev, tid, i_buffer):
    if hasattr(dev, 'tracer_get_buffer'):
        return dev.tracer_get_buffer(tid, i_buffer)
    return dev.tracers[tid]['T'][i_buffer].copy()              # tests/cpu_device.py


# ---- cell ranges --------------------------------------------------------------------------------------------------------------------
def split_points(n):
    """cuts at the first and last cell and around the ends of the first two 64-cell workgroups"""
    if n < SPLIT_FROM:
        raise ValueError('split_points: at least {} cells'.format(SPLIT_FROM))
    return sorted(set([0, 1, 63, 64, 65, 127, 129, n - 1, n]))


def split_ranges(n):
    """the ranges between the cuts and one empty range, in a fixed shuffled order"""
    cuts = split_points(n)
    ranges = list(zip(cuts[:-1], cuts[1:])) + [(64, 64)]
    return [ranges[i] for i in np.random.default_rng(2024).permutation(len(ranges))]


def whole(n):
    return [(0, n)]


def run_stages(dev, ranges):
    """the three stages, each over ``ranges``: the stage solutions [(uv, eta)] * 3"""
    out = []
    for i in range(3):
        for a, b in ranges:
            dev.solve_stage_cells(i, a, b)
        out.append(dev.get_state(i))
    return out


def run_forward_euler(dev, ranges):
    for a, b in ranges:
        dev.forward_euler_cells(a, b)
    dev.swap_state_buffers()
    return dev.get_state()


def run_tracer_stages(dev, tid, ranges):
    """the buffers tracer stages 0, 1, 2 wrote (1, 2, 0)"""
    out = []
    for i in range(3):
        for a, b in ranges:
            dev.tracer_solve_stage_cells(tid, i, a, b)
        out.append(tracer_buffer(dev, tid, (i + 1) % 3))
    return out


def same_bits(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def compare_split(dev_whole, dev_split, uv, eta, T, tid_whole, tid_split, what=None):
    """every stage, the ForwardEuler step, every tracer stage and the limiter: once over [0, n) on ``dev_whole``, range by range on the
    identical ``dev_split`` - the same bits"""
    n = dev_whole.n_cells
    ranges = split_ranges(n)
    assert sorted(r for r in ranges if r[0] < r[1]) == list(zip(split_points(n)[:-1], split_points(n)[1:])) and (64, 64) in ranges
    for dev in (dev_whole, dev_split):
        dev.set_state(uv, eta)
    for i, (ref, got) in enumerate(zip(run_stages(dev_whole, whole(n)), run_stages(dev_split, ranges))):
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all(), ('stage', i, what)
        assert np.abs(ref[1] - eta).max() > 0.0, ('stage', i, what)
        assert same_bits(ref, got), ('stage', i, first_difference(ref, got), what)
    for dev in (dev_whole, dev_split):
        dev.set_state(uv, eta)
    ref, got = run_forward_euler(dev_whole, whole(n)), run_forward_euler(dev_split, ranges)
    assert np.isfinite(ref[0]).all() and np.abs(ref[1] - eta).max() > 0.0, ('forward_euler', what)
    assert same_bits(ref, got), ('forward_euler', first_difference(ref, got), what)
    for dev, tid in ((dev_whole, tid_whole), (dev_split, tid_split)):
        dev.set_state(uv, eta)
        dev.tracer_set_state(tid, T)
    for i, (ref, got) in enumerate(zip(run_tracer_stages(dev_whole, tid_whole, whole(n)), run_tracer_stages(dev_split, tid_split, ranges))):
        assert np.isfinite(ref).all() and np.abs(ref - T).max() > 0.0, ('tracer stage', i, what)
        assert same_bits(ref, got), ('tracer stage', i, first_difference((ref,), (got,)), what)
    for dev, tid in ((dev_whole, tid_whole), (dev_split, tid_split)):
        dev.tracer_set_state(tid, T)
    dev_whole.tracer_limit(tid_whole)
    dev_split.tracer_limit_cells(tid_split, n)
    ref, got = dev_whole.tracer_get_state(tid_whole), dev_split.tracer_get_state(tid_split)
    assert np.abs(ref - T).max() > 0.0, ('limiter', what)
    assert same_bits(ref, got), ('limiter', first_difference((ref,), (got,)), what)


def first_difference(a, b):
    bad = np.zeros(len(a[0]), dtype=bool)
    for x, y in zip(a, b):
        bad |= (x != y).reshape(len(x), -1).any(axis=1)
    rows = np.nonzero(bad)[0]
    return 'no cell differs' if len(rows) == 0 else '{} cells differ (caller numbering), the first {}'.format(len(rows), rows[:8])


# ---- cells outside a range ----------------------------------------------------------------------------------------------------------
OUTSIDE_RANGES = [(1, 63), (63, 65), (64, 130), (129, 130)]
LIMIT_ENDS = [1, 64, 65, 129]


def caller_cells(dev, a, b):
    """the caller's numbers of the device cells [a, b)"""
    perm = getattr(dev, 'perm', None)
    return np.arange(a, b) if perm is None else np.asarray(perm)[a:b]


def check_outside(dev, a, b, got, full, before, what=None, must_change=True):
    """``got``: cells [a, b) of the device hold ``full`` (the whole launch), every other cell ``before`` - to the bit"""
    n = len(got[0]) if isinstance(got, tuple) else len(got)
    inside = caller_cells(dev, a, b)
    outside = np.setdiff1d(np.arange(n), inside)
    assert len(inside) == b - a and len(outside) == n - (b - a)
    pick = lambda s, rows: tuple(x[rows] for x in s) if isinstance(s, tuple) else s[rows]
    assert same_bits(pick(got, inside), pick(full, inside)), ('cells of the range differ from the whole launch', a, b, what)
    assert same_bits(pick(got, outside), pick(before, outside)), ('cells outside the range changed', a, b, what)
    # (the limiter leaves a cell inside its vertex bounds alone: that it acts at all is asserted on the whole mesh)
    assert not must_change or not same_bits(pick(full, inside), pick(before, inside)), ('the stage changes nothing', a, b, what)


def stage_2_on_range(dev, uv, eta, a, b):
    """stages 0 and 1 over the whole mesh, stage 2 - which writes the state in place - on [a, b) only"""
    dev.set_state(uv, eta)
    dev.solve_stage(0)
    dev.solve_stage(1)
    dev.solve_stage_cells(2, a, b)
    return dev.get_state()


def tracer_stage_2_on_range(dev, tid, T, a, b):
    dev.tracer_set_state(tid, T)
    dev.tracer_solve_stage(tid, 0)
    dev.tracer_solve_stage(tid, 1)
    dev.tracer_solve_stage_cells(tid, 2, a, b)
    return dev.tracer_get_state(tid)


def check_outside_ranges(dev, tid, uv, eta, T, what=None):
    """stage 2 and tracer stage 2 on each of OUTSIDE_RANGES, the limiter up to each of LIMIT_ENDS: the range gets the whole launch's
    bits, every other cell keeps what was set"""
    n = dev.n_cells
    full = stage_2_on_range(dev, uv, eta, 0, n)
    set_ = (np.asarray(uv, dtype=np.float64), np.asarray(eta, dtype=np.float64))
    for a, b in OUTSIDE_RANGES:
        check_outside(dev, a, b, stage_2_on_range(dev, uv, eta, a, b), full, set_, ('stage 2', what))
    dev.set_state(uv, eta)
    full = tracer_stage_2_on_range(dev, tid, T, 0, n)
    for a, b in OUTSIDE_RANGES:
        check_outside(dev, a, b, tracer_stage_2_on_range(dev, tid, T, a, b), full, T, ('tracer stage 2', what))
    dev.tracer_set_state(tid, T)
    dev.tracer_limit(tid)
    full = dev.tracer_get_state(tid)
    assert np.abs(full - T).max() > 0.0, ('the limiter changes nothing', what)
    for m in LIMIT_ENDS:
        dev.tracer_set_state(tid, T)
        dev.tracer_limit_cells(tid, m)
        check_outside(dev, 0, m, dev.tracer_get_state(tid), full, T, ('limiter', what), must_change=False)
