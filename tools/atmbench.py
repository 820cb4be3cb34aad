"""ms per time step of FlowSolver2d.iterate with wind stress and atmospheric pressure over a closed basin (thetis_amd/forcing.py,
csrc/swe2d_atm.hip):
(a) wind stress and pressure fields that are constant in time, the handle kept on stage launches (SWE2D_OPT_FUSED_STAGES = 0,
    SWE2D_OPT_FLOW = 0): what (b) adds its three evaluation launches per step to;
(b) the record of snapshots evaluated on the device, the steps batched;
(c) the same record through ``update_forcings`` + ``set_fields``: Python, two per-vertex uploads and one stage launch per stage.
Then swe_atm_kernel alone: ``--kernel-calls`` back-to-back ``atm_eval`` calls, us per launch and GB/s on the byte model
3*NPC*8 B written + 4*NPC B of cv + 48 B gathered per vertex (half a vertex per triangle) per cell.

    python tools/atmbench.py [--nx 707 --ny 707] [--steps 200]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  Each case
is timed ``--repeats`` times in the same process, one after the other; the median is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import AtmosphericForcing, Constant, Function, RectangleMesh, _lib, get_functionspace, solver2d  # noqa: E402

N_SNAPSHOTS = 4


def build(nx, ny, case, t_span):
    lx, ly = 100e3, 100e3*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    P1 = get_functionspace(mesh, 'CG', 1)
    s = solver2d.FlowSolver2d(mesh, Function(P1).interpolate(lambda x, y: 20.0 - 10.0*x/lx))
    o = s.options
    o.timestep = 0.05*(lx/nx)/np.sqrt(9.81*20.0)
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.output_directory = os.path.join('outputs', 'atmbench')
    x, y = mesh.vertex_xy[:, 0]/lx, mesh.vertex_xy[:, 1]/ly
    times = np.linspace(0.0, t_span*o.timestep, N_SNAPSHOTS)
    u = np.stack([(10.0 + 5.0*k)*np.cos(2.0*y + 0.3*k)*(0.2 + x) for k in range(N_SNAPSHOTS)])
    v = np.stack([(10.0 + 5.0*k)*np.sin(2.0*y + 0.3*k)*(0.2 + x) for k in range(N_SNAPSHOTS)])
    p = np.stack([101325.0 - 1500.0*np.exp(-((x - 0.2 - 0.2*k)**2 + (y - 0.5)**2)/0.05) for k in range(N_SNAPSHOTS)])
    f = AtmosphericForcing(Function(get_functionspace(mesh, 'CG', 1, vector=True)), Function(P1), times, u, v, p)
    if case == 'b':
        o.wind_stress, o.atmospheric_pressure = f, f
    else:
        f.set_fields(0.0)
        o.wind_stress, o.atmospheric_pressure = f.wind_stress_field, f.atm_pressure_field
    s.assign_initial_conditions(elev=Constant(0.0))
    if case == 'a':
        s.timestepper.device.set_option(_lib.OPT_FUSED_STAGES, 0)
        s.timestepper.device.set_option(_lib.OPT_FLOW, 0)
    s.print_state = lambda *a, **k: None
    return s, f


def run(nx, ny, steps, case, warmup, repeats):
    s, f = build(nx, ny, case, warmup + steps*repeats + 2)
    o = s.options
    forcings = f.set_fields if case == 'c' else None

    def batch(n):
        o.simulation_export_time = n*o.timestep
        o.simulation_end_time = s.simulation_time + (n - 0.5)*o.timestep
        s.export_initial_state = False
        t0 = time.perf_counter()
        s.iterate(update_forcings=forcings)
        s.timestepper.device.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    batch(warmup)
    return float(np.median([batch(steps) for _ in range(repeats)]))


def kernel_alone(nx, ny, calls, repeats):
    """us per swe_atm_kernel launch: ``calls`` back-to-back atm_eval calls between two synchronisations"""
    s, f = build(nx, ny, 'b', 10)
    dev = s.timestepper.device
    t_mid = 0.37*float(f.times[-1])
    for _ in range(10):
        dev.atm_eval(t_mid)
    dev.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            dev.atm_eval(t_mid)
        dev.synchronize()
        out.append(1e6*(time.perf_counter() - t0)/calls)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='abc')
    ap.add_argument('--kernel-calls', type=int, default=100)
    args = ap.parse_args()
    n_cells = 2*args.nx*args.ny
    res = {'cells': n_cells, 'steps': args.steps, 'repeats': args.repeats}
    for c in args.cases:
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.steps, c, args.warmup, args.repeats)
    if 'ms_per_step_a' in res and 'ms_per_step_b' in res:
        res['b_over_a'] = res['ms_per_step_b']/res['ms_per_step_a']
    if 'ms_per_step_b' in res and 'ms_per_step_c' in res:
        res['c_over_b'] = res['ms_per_step_c']/res['ms_per_step_b']
    if args.kernel_calls > 0:
        us = kernel_alone(args.nx, args.ny, args.kernel_calls, args.repeats)
        model_bytes = n_cells*(3*3*8 + 4*3 + 0.5*48)
        res['atm_kernel_us'] = us
        res['atm_kernel_gb_per_s'] = model_bytes/(us*1e-6)/1e9
        res['atm_kernel_fraction_of_8_tb_per_s'] = res['atm_kernel_gb_per_s']/8000.0
    print(json.dumps(res))


if __name__ == '__main__':
    main()
