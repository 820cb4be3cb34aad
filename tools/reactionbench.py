"""ms per time step of FlowSolver2d.iterate with two P1DG tracers, tracer_only, SSPRK33 (thetis_amd/reactions.py,
csrc/swe2d_reaction.hip):
(a)  two tracers without sources;
(b)  the Gray-Scott sources, evaluated on the device in front of every stage (the batched coupled step);
(c)  the Gray-Scott sources through the per-stage host fallback: a device class without ``tracer_set_reaction`` - the stepper pulls
     the tracers per stage, evaluates ``HostReaction`` in numpy and uploads the source (two transfers of a field and an upload per stage);
and the pass alone: ms per stage launch of 100 launches back to back with the program, minus the same launches with the same planes
as an uploaded (frozen) source - the stage kernel is the same SRC instance in both, the difference is swe_reaction_kernel.  Per cell
the pass reads the 3 nodal values of each of its 2 tracer operands once from memory (48 B; the 8 further quadrature points re-read
them from cache) and writes 3 source values (24 B): 72 B per cell, reported against its time as GB/s.

    python tools/reactionbench.py [--nx 707 --ny 707] [--steps 100] [--host-steps 5]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  All cases
of a mesh run in the same process, one after the other, each ``--repeats`` times; the median is reported.  The host case takes
``--host-steps`` steps per repeat."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, Function, RectangleMesh, get_functionspace, solver2d  # noqa: E402
from thetis_amd.device import Swe2dDevice  # noqa: E402

GAMMA, KAPPA = 0.024, 0.06
BYTES_PER_CELL = 2*3*8 + 3*8


class HostFallbackDevice(Swe2dDevice):
    """the device without the reaction calls: the stepper takes the per-stage host evaluation"""

    @property
    def tracer_set_reaction(self):
        raise AttributeError('tracer_set_reaction')


def make_solver(nx, ny, case):
    lx, ly = 100e3, 100e3*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    s = solver2d.FlowSolver2d(mesh, Function(get_functionspace(mesh, 'CG', 1)).assign(10.0))
    if case == 'c':
        s._device_cls = HostFallbackDevice
    o = s.options
    o.tracer_only = True
    o.use_limiter_for_tracers = False
    o.no_exports = True
    o.output_directory = os.path.join('outputs', 'reactionbench')
    o.swe_timestepper_type = 'SSPRK33'
    o.tracer_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.tracer_timestepper_options.use_automatic_timestep = False
    o.timestep = 0.05*(lx/nx)/0.5                       # a twentieth of the advective limit of the 0.5 m/s below; k*dt << 1
    P1DG = get_functionspace(mesh, 'DG', 1)
    a, b = Function(P1DG, name='a_2d'), Function(P1DG, name='b_2d')
    g, k = Constant(GAMMA/o.timestep/50.0), Constant(KAPPA/o.timestep/50.0)     # rates scaled to the step: the same work, bounded values
    src = (None, None) if case == 'a' else (g - g*a*b**2 - g*a, g*a*b**2 - (g + k)*b)
    o.add_tracer_2d('a_2d', 'Tracer A', 'TracerA2d', function=a, source=src[0])
    o.add_tracer_2d('b_2d', 'Tracer B', 'TracerB2d', function=b, source=src[1])
    rng = np.random.default_rng(1)
    shape = a.dat.data_ro.shape
    s.assign_initial_conditions(uv=lambda x, y: (0.5 + 0*x, 0.0*x), a=Function(P1DG).assign(rng.uniform(0.2, 1.0, size=shape)),
                                b=Function(P1DG).assign(rng.uniform(0.2, 1.0, size=shape)))
    s.print_state = lambda *a, **k: None
    ti = s.timestepper
    assert len(ti.reacting) == (0 if case == 'a' else 2) and ti.host_reactions == (case == 'c')
    return s


def run(nx, ny, steps, case, warmup, repeats):
    s = make_solver(nx, ny, case)
    o = s.options

    def batch(n):
        o.simulation_export_time = n*o.timestep
        o.simulation_end_time = s.simulation_time + (n - 0.5)*o.timestep
        s.export_initial_state = False
        t0 = time.perf_counter()
        s.iterate()
        s.timestepper.device.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    batch(warmup)
    out = float(np.median([batch(steps) for _ in range(repeats)]))
    assert np.isfinite(s.fields.a_2d.dat.data_ro).all()
    s.timestepper.device.close()
    return out


def pass_alone(nx, ny, launches, repeats):
    """ms per launch of the reaction pass: stage launches with the program minus the same with its planes as a frozen source"""
    s = make_solver(nx, ny, 'b')
    dev = s.timestepper.device
    for ts in s.timestepper.tracers.values():
        ts._sync_to_device()

    def burst(n):
        dev.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            dev.tracer_solve_stage(0, 0)
        dev.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    burst(10)
    with_pass = float(np.median([burst(launches) for _ in range(repeats)]))
    dev.tracer_set_source(0, dev.tracer_get_source(0))          # the same planes, uploaded: the program is gone
    burst(10)
    without = float(np.median([burst(launches) for _ in range(repeats)]))
    dev.close()
    return with_pass, without


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--host-steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='a,b,c')
    args = ap.parse_args()
    cells = 2*args.nx*args.ny
    res = {'cells': cells, 'steps': args.steps, 'host_steps': args.host_steps, 'repeats': args.repeats}
    for c in args.cases.split(','):
        host = c == 'c'
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.host_steps if host else args.steps, c,
                                      min(args.warmup, 2) if host else args.warmup, args.repeats)
    with_pass, without = pass_alone(args.nx, args.ny, 100, args.repeats)
    ms = with_pass - without
    res.update({'stage_ms_with_pass': with_pass, 'stage_ms_frozen_source': without, 'pass_ms': ms,
                'pass_bytes_per_cell': BYTES_PER_CELL, 'pass_GBps': cells*BYTES_PER_CELL/(1e6*ms) if ms > 0 else None})
    if 'ms_per_step_a' in res and 'ms_per_step_b' in res:
        res['b_minus_a_ms_per_step'] = res['ms_per_step_b'] - res['ms_per_step_a']
    if 'ms_per_step_b' in res and 'ms_per_step_c' in res:
        res['c_over_b'] = res['ms_per_step_c']/res['ms_per_step_b']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
