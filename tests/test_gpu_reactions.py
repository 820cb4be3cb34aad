"""Reacting tracers on the device (csrc/swe2d_reaction.hip): the nodal source the pass writes against the independent replay of
tests/reaction_cases.py bit for bit - per stage, on four meshes, for three programs and for a program at every limit -; the stepping
paths (coupled batches, ForwardEuler, conservative form, wetting-drying, diffusion fused and unfused) against a stage-by-stage loop
on the same handle bit for bit and against the host stand-in through the oracle; FlowSolver2d's batches; SQRT / EXP / LOG in ulps."""
import numpy as np
import pytest

from helpers import quad_case, rel_linf
from particle_cases import scenario
from reaction_cases import (GAMMA, KAPPA, ReactionCpuDevice, channel520, gray_scott_solver, gs_a, gs_b, replay_np, run_postfix_np,
                            word)
from thetis_amd import (Constant, DetectorsCallback, Function, RectangleMesh, SpatialCoordinate, _lib, conditional, exp,
                        get_functionspace, gt, ln, max_value, reactions, sqrt)
from thetis_amd.device import Swe2dDevice
from thetis_amd.function import farm_quadrature

pytestmark = pytest.mark.gpu
TOL = 1e-12                     # tests/test_gpu_tracer.py: sourced tracers against the oracle
K_MONOD = 0.3


def _mesh(name):
    if name == 'square2':
        return RectangleMesh(1, 1, 10.0, 10.0), 1.0
    if name == 'channel':
        mesh, bath, _, _ = channel520()
        return mesh, bath
    if name == 'coast':
        mesh, bath = scenario('coast')[:2]
        return mesh, bath
    mesh, bath, _, _ = quad_case(nx=6, ny=5, skew=0.3)
    assert mesh.affine
    return mesh, bath


def _programs(mesh):
    """name -> [(expression of tracer a, replay function), (of tracer b, ...)] on Functions a, b (tracer ids 0, 1)"""
    P1DG = get_functionspace(mesh, 'DG', 1)
    a, b = Function(P1DG), Function(P1DG)
    ids = {id(a): 0, id(b): 1}
    x, _ = SpatialCoordinate(mesh)
    L = float(np.abs(mesh.vertex_xy[:, 0]).max())
    g, k = Constant(GAMMA), Constant(KAPPA)
    progs = {
        'gray_scott': [(g - a*b**2 - g*a, gs_a), (a*b**2 - (g + k)*b, gs_b)],
        'monod': [(-0.05*(a*b/(K_MONOD + a)), lambda v: -0.05*(v['a']*v['b']/(K_MONOD + v['a']))),
                  (0.02*(a*b/(K_MONOD + a)), lambda v: 0.02*(v['a']*v['b']/(K_MONOD + v['a'])))],
        'conditional': [(conditional(gt(a, b), max_value(a, b)*x/L, -b)*0.05,
                         lambda v: np.where(v['a'] > v['b'], np.where(v['b'] > v['a'], v['b'], v['a'])*v['x']/L, -v['b'])*0.05),
                        (0.01*abs(a - b), lambda v: 0.01*np.abs(v['a'] - v['b']))],
    }
    return progs, (lambda f: ids.get(id(f)))


def _device(mesh, bath, dt=0.5, seed=0, flow=0.0):
    bathv = np.full(mesh.num_vertices, float(bath)) if np.isscalar(bath) else np.asarray(bath)
    dev = Swe2dDevice(mesh, bathv, dt, boundary_len=mesh.boundary_len)
    npc = mesh.cells.shape[1]
    rng = np.random.default_rng(seed)
    dev.set_state(flow*rng.normal(size=(mesh.num_cells, npc, 2)), 0.1*flow*rng.normal(size=(mesh.num_cells, npc)))
    for tid in range(2):
        assert dev.add_tracer() == tid
        dev.tracer_set_state(tid, rng.uniform(0.2, 1.0, size=(mesh.num_cells, npc)))
    return dev


def _set_programs(dev, mesh, pair, tracer_of):
    out = []
    for tid, (src, fn) in enumerate(pair):
        p = reactions.compile_source(src, tracer_of, npc=mesh.cells.shape[1])
        dev.tracer_set_reaction(tid, p.code, p.constant_values(), p.phi, p.w)
        out.append((p, fn))
    return out


def _operands(dev, mesh, tid, i_in):
    return {'a': dev.tracer_get_buffer(0, i_in if tid == 0 else 0), 'b': dev.tracer_get_buffer(1, i_in if tid == 1 else 0),
            'x': mesh.cell_xy()[:, :, 0], 'y': mesh.cell_xy()[:, :, 1]}


@pytest.mark.parametrize('prog', ['gray_scott', 'monod', 'conditional'])
@pytest.mark.parametrize('name', ['square2', 'channel', 'coast', 'quads'])
def test_source_bits(hip_lib, name, prog):
    """swe2d_tracer_get_source after every stage of 3 steps equals the replay from the buffers the stage read, bit for bit"""
    mesh, bath = _mesh(name)
    dev = _device(mesh, bath, flow=0.05)
    progs, tracer_of = _programs(mesh)
    ps = _set_programs(dev, mesh, progs[prog], tracer_of)
    if prog == 'gray_scott':
        assert ps[0][0].phi.shape == (9, mesh.cells.shape[1])
    seen = 0.0
    for step in range(3):
        for tid, (p, fn) in enumerate(ps):
            for i in range(3):
                want = replay_np(p.phi, p.w, _operands(dev, mesh, tid, i), fn)
                dev.tracer_solve_stage(tid, i)
                got = dev.tracer_get_source(tid)
                assert np.array_equal(got, want), (name, prog, step, tid, i, np.abs(got - want).max())
                seen = max(seen, np.abs(got).max())
    assert seen > 1e-4 and np.isfinite(dev.tracer_get_state(0)).all()
    dev.close()


def _limit_program(mesh):
    """64 instructions, 8 values on the stack, 16 constants, 4 coefficient fields, a 64-point rule"""
    code = [word('FIELD', 0), word('FIELD', 1), word('FIELD', 2), word('FIELD', 3), word('TRACER', 0), word('TRACER', 1),
            word('CONST', 0), word('CONST', 1)]
    code += [word(n) for n in ('MUL', 'ADD', 'MUL', 'ADD', 'MUL', 'ADD', 'SUB')]
    for i in range(2, 16):
        code += [word('CONST', i), word('MUL' if i % 2 else 'ADD')]
    for i in range(10):
        code += [word('TRACER', i % 2), word('SUB' if i % 2 else 'ADD')]
    code += [word('NEG')]
    assert len(code) == 64
    consts = np.linspace(0.9, 1.1, 16)
    phi, w = farm_quadrature(3, 14)
    assert len(w) == 64
    return np.array(code, dtype=np.int32), consts, phi, w


def test_program_at_every_limit(hip_lib):
    mesh, bath = _mesh('channel')
    dev = _device(mesh, bath)
    code, consts, phi, w = _limit_program(mesh)
    P1, P1DG = get_functionspace(mesh, 'CG', 1), get_functionspace(mesh, 'DG', 1)
    rng = np.random.default_rng(4)
    fields = []
    for slot, fs in enumerate((P1, P1DG, P1, P1DG)):            # CG and DG coefficient Functions
        f = Function(fs).assign(rng.uniform(0.5, 1.5, size=fs.node_count()))
        fields.append(np.array(f.cell_node_values()))
        dev.reaction_set_field(slot, fields[-1])
    dev.tracer_set_reaction(0, code, consts, phi, w)
    ops = _operands(dev, mesh, 0, 0)
    ops.update({'f{:d}'.format(i): f for i, f in enumerate(fields)})
    names, fnames = {0: 'a', 1: 'b'}, {i: 'f{:d}'.format(i) for i in range(4)}
    want = replay_np(phi, w, ops, lambda v: run_postfix_np(code, consts, v, names, fnames))
    dev.tracer_solve_stage(0, 0)
    got = dev.tracer_get_source(0)
    assert np.array_equal(got, want) and np.abs(got).max() > 0.1
    # one beyond each limit is refused and the handle stays usable
    for bad in (lambda: dev.tracer_set_reaction(0, np.append(code, word('NEG')), consts, phi, w),
                lambda: dev.tracer_set_reaction(0, code, np.append(consts, 1.0), phi, w),
                lambda: dev.tracer_set_reaction(0, [word('TRACER', 0)]*9 + [word('ADD')]*8, consts, phi, w),
                lambda: dev.tracer_set_reaction(0, [word('TRACER', 0), word('ADD')], consts, phi, w),
                lambda: dev.tracer_set_reaction(0, [word('TRACER', 5)], consts, phi, w),
                lambda: dev.tracer_set_reaction(0, [word('CONST', 16)], consts, phi, w),
                lambda: dev.tracer_set_reaction(0, [word('FIELD', 4)], consts, phi, w),
                lambda: dev.tracer_set_reaction(0, [word('TRACER', 0), word('POWI', 17)], consts, phi, w)):
        with pytest.raises(_lib.Swe2dError) as err:
            bad()
        assert err.value.code == _lib.ERR_INVALID_ARGUMENT
    dev.tracer_solve_stage(0, 1)
    assert np.isfinite(dev.tracer_get_source(0)).all()
    dev.tracer_set_reaction(0, None)                           # removed: no source again
    with pytest.raises(_lib.Swe2dError):
        dev.tracer_get_source(0)
    dev.close()


def test_general_quadrilaterals_are_unsupported(hip_lib):
    mesh, bath, _, _ = quad_case(nx=4, ny=3, warp=0.2)
    dev = _device(mesh, bath)
    phi, w = farm_quadrature(4, 2)
    with pytest.raises(_lib.Swe2dError) as err:
        dev.tracer_set_reaction(0, [word('TRACER', 0)], [], phi, w)
    assert err.value.code == _lib.ERR_UNSUPPORTED
    dev.tracer_solve_stage(0, 0)
    assert np.isfinite(dev.tracer_get_buffer(0, 1)).all()
    dev.close()


# ---- stepping paths: the batched call against a stage-by-stage loop on the same handle
def _configure(dev, variant):
    if variant == 'conservative':
        dev.tracer_set_conservative(0, True)
        dev.tracer_set_conservative(1, True)
    if variant == 'wetting_drying':
        uv, eta = dev.get_state()
        dev.set_wetting_and_drying(0.5)
        dev.set_state(uv, eta)                  # (the state is brought to the admissible set)
    if variant in ('diffusion', 'diffusion_unfused'):
        dev.tracer_set_diffusivity(0, 8.0, 1.0)
        dev.tracer_set_diffusivity(1, 4.0, 1.0)
    if variant == 'diffusion_unfused':
        dev.set_option(_lib.OPT_VISC_FUSION, 0)


@pytest.mark.parametrize('variant', ['plain', 'forward_euler', 'conservative', 'wetting_drying', 'diffusion', 'diffusion_unfused'])
def test_stepping_paths(hip_lib, variant):
    """3 steps in one swe2d_advance_coupled (limiter on, the tracers advected by a non-zero velocity) against the loop over
    swe2d_tracer_solve_stage + swe2d_tracer_limit from the same snapshot: bit for bit, and the source of the last stage is the
    replay's.  ForwardEuler: swe2d_tracer_forward_euler against stage 0 + swap."""
    mesh, bath = _mesh('channel')
    # (the conservative form multiplies the source by the depth, 5 - 20 m here: a step the explicit scheme is stable with)
    dev = _device(mesh, bath, dt=0.05 if variant == 'conservative' else 2.0, flow=0.3)
    _configure(dev, variant)
    progs, tracer_of = _programs(mesh)
    ps = _set_programs(dev, mesh, progs['gray_scott'], tracer_of)
    dev.snapshot()
    start = [dev.tracer_get_state(t) for t in range(2)]
    if variant == 'forward_euler':
        for _ in range(3):
            for tid in range(2):
                dev.tracer_forward_euler(tid)
    else:
        dev.advance_coupled(3, tracer_only=True, use_limiter=True)
    batched = [dev.tracer_get_state(t) for t in range(2)]
    dev.restore()
    assert all(np.array_equal(dev.tracer_get_state(t), start[t]) for t in range(2))
    for step in range(3):
        for tid, (p, fn) in enumerate(ps):
            if variant == 'forward_euler':
                want = replay_np(p.phi, p.w, _operands(dev, mesh, tid, 0), fn)
                dev.tracer_solve_stage_cells(tid, 0, 0, mesh.num_cells)
                dev.tracer_swap_buffers(tid)
            else:
                for i in range(3):
                    want = replay_np(p.phi, p.w, _operands(dev, mesh, tid, i), fn)
                    dev.tracer_solve_stage(tid, i)
                dev.tracer_limit(tid)
            assert np.array_equal(dev.tracer_get_source(tid), want)
    for t in range(2):
        got = dev.tracer_get_state(t)
        assert np.array_equal(got, batched[t]), (variant, t, np.abs(got - batched[t]).max())
        assert np.abs(got - start[t]).max() > 1e-3 and np.isfinite(got).all() and np.abs(got).max() < 10.0
    dev.close()


def test_flow_on_batches_and_the_host_fallback(hip_lib):
    """with the shallow-water step in the batch: 3 steps in one call equal 3 calls of one step bit for bit; and the device's two
    steps (frozen flow, no limiter) against the host stand-in stepping through the oracle with replayed sources, to the tolerance
    of the sourced tracers of tests/test_gpu_tracer.py"""
    mesh, bath = _mesh('channel')
    dev = _device(mesh, bath, dt=2.0, flow=0.3)
    progs, tracer_of = _programs(mesh)
    ps = _set_programs(dev, mesh, progs['gray_scott'], tracer_of)
    dev.snapshot()
    uv0, eta0 = dev.get_state()
    start = [dev.tracer_get_state(t) for t in range(2)]
    dev.advance_coupled(3, tracer_only=False, use_limiter=True)
    one = [dev.tracer_get_state(t) for t in range(2)] + list(dev.get_state())
    dev.restore()
    for _ in range(3):
        dev.advance_coupled(1, tracer_only=False, use_limiter=True)
    for a, b in zip(one, [dev.tracer_get_state(t) for t in range(2)] + list(dev.get_state())):
        assert np.array_equal(a, b)
    assert np.abs(one[3] - eta0).max() > 1e-6
    # host stand-in: the oracle's tracer stage with the replayed source
    dev.restore()
    dev.advance_coupled(2, tracer_only=True, use_limiter=False)
    cpu = ReactionCpuDevice(mesh, bath, 2.0, boundary_len=mesh.boundary_len)
    cpu.set_state(uv0, eta0)
    for t in range(2):
        cpu.add_tracer()
        cpu.tracer_set_state(t, start[t])
    for step in range(2):
        for tid, (p, fn) in enumerate(ps):
            for i in range(3):
                ops = {'a': cpu.tracer_get_buffer(0, i if tid == 0 else 0), 'b': cpu.tracer_get_buffer(1, i if tid == 1 else 0)}
                cpu.tracer_set_source(tid, replay_np(p.phi, p.w, ops, fn))
                cpu.tracer_solve_stage(tid, i)
    for t in range(2):
        err = rel_linf(dev.tracer_get_state(t), cpu.tracer_get_state(t))
        print('device against the host stand-in, tracer', t, err)
        assert err < TOL
    dev.close()


# ---- FlowSolver2d
N_STEPS = 12


def _solver_run(mode, with_detectors=False, tmp='.'):
    mesh = channel520()[0]
    so = gray_scott_solver(mesh, tmp, 2.0, N_STEPS, diffusivity=(8.0, 4.0))
    so.assign_initial_conditions(uv=lambda x, y: (0.3 + 0*x, 0.1 + 0*x), **so._ic)
    det = None
    if with_detectors:
        det = DetectorsCallback(so, [(30e3, 11e3), (71e3, 19e3)], ['a_2d'], 'gauges', export_to_hdf5=False)
        so.add_callback(det, eval_interval='timestep')
    ti = so.timestepper
    assert len(ti.reacting) == 2 and not ti.host_reactions
    dev = ti.device
    calls, stage_calls = [], []
    inner, inner_stage = dev.advance_coupled, dev.tracer_solve_stage
    dev.advance_coupled = lambda n=1, **kw: (calls.append(int(n)), inner(n, **kw))[1]
    dev.tracer_solve_stage = lambda tid, i: (stage_calls.append(tid), inner_stage(tid, i))[1]
    if mode == 'iterate':
        so.iterate()
    else:
        for _ in so.create_iterator():
            pass
    assert so.iteration == N_STEPS and not stage_calls
    out = {'calls': calls, 'a': so.fields.a_2d.dat.data_ro.copy(), 'b': so.fields.b_2d.dat.data_ro.copy(), 'a0': so._ab0[0]}
    if det is not None:
        out['rows'] = np.array([h[0] for h in det.history])
    del dev.advance_coupled, dev.tracer_solve_stage             # (the counting wrappers hold the device's own methods: no cycle left)
    dev.close()
    return out


def test_iterate_keeps_its_batches(hip_lib, tmp_path):
    batched = _solver_run('iterate', tmp=str(tmp_path/'a'))
    loop = _solver_run('loop', tmp=str(tmp_path/'b'))
    assert batched['calls'] == [N_STEPS] and loop['calls'] == [1]*N_STEPS
    assert np.array_equal(batched['a'], loop['a']) and np.array_equal(batched['b'], loop['b'])
    assert np.abs(batched['a'] - batched['a0']).max() > 1e-3
    with_rows = _solver_run('iterate', with_detectors=True, tmp=str(tmp_path/'c'))
    rows_loop = _solver_run('loop', with_detectors=True, tmp=str(tmp_path/'d'))
    assert with_rows['calls'] == [1]*N_STEPS                                   # a row per step: a call per step, none by stages
    assert with_rows['rows'].shape[0] == N_STEPS and np.array_equal(with_rows['rows'], rows_loop['rows'])
    assert np.array_equal(with_rows['a'], batched['a'])


# ---- the device's math library
# largest difference to the replay (numpy's functions), in ulps of the largest source value, measured on an MI355X over this test's
# inputs; SQRT is correctly rounded on both sides: no room
ULP_MEASURED = {'sqrt': 0.0, 'exp': 0.5, 'ln': 2.0}


@pytest.mark.parametrize('fname', ['sqrt', 'exp', 'ln'])
def test_sqrt_exp_log_in_ulps(hip_lib, fname):
    """SQRT, EXP, LOG with arguments in [1e-3, 10]: the device's math library need not round as numpy does; the bound is 4 times
    the largest difference measured on an MI355X (Reacting tracers), a structural error shows at 1e-3 relative."""
    mesh, bath = _mesh('channel')
    dev = _device(mesh, bath)
    rng = np.random.default_rng(9)
    va = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), size=(mesh.num_cells, 3)))
    dev.tracer_set_state(0, va)
    P1DG = get_functionspace(mesh, 'DG', 1)
    a = Function(P1DG)
    f, nf = {'sqrt': (sqrt, np.sqrt), 'exp': (exp, np.exp), 'ln': (ln, np.log)}[fname]
    p = reactions.compile_source(f(a), lambda g: 0 if g is a else None)
    dev.tracer_set_reaction(0, p.code, p.constant_values(), p.phi, p.w)
    want = replay_np(p.phi, p.w, {'a': va}, lambda v: nf(v['a']))
    dev.tracer_solve_stage(0, 0)
    got = dev.tracer_get_source(0)
    ulps = float(np.abs(got - want).max()/np.spacing(np.abs(want).max()))
    print('ulps', fname, ulps, 'relative', rel_linf(got, want))
    assert rel_linf(got, want) < 1e-3
    assert ulps <= 4.0*ULP_MEASURED[fname]
    dev.close()
