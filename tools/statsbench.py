"""ms per time step of FlowSolver2d.iterate with running field statistics (thetis_amd/fieldstats.py, csrc/swe2d_stats.hip), K = 8
harmonic constituents:
(a)   no callback;
(b1)  FieldStatisticsCallback on the device, every = 1;      (b10)  the same with every = 10;
(c1)  a host callback that reads elev_2d and uv_2d at every sampled step and does the same numpy updates, every = 1;   (c10)  every = 10;
and the statistics kernel alone: ms per append and the bytes per second it reaches on its own byte model, 24 B read and
16*(8 + 2K) B read-modified-written per node and sample.

    python tools/statsbench.py [--nx 707 --ny 707] [--steps 200]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  Each case
is timed ``--repeats`` times in the same process, one after the other; the median is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, FieldStatisticsCallback, Function, RectangleMesh, get_functionspace, solver2d  # noqa: E402
from thetis_amd.callback import DiagnosticCallback  # noqa: E402
from thetis_amd.fieldstats import HostFieldStats, harmonic_weights  # noqa: E402

HBM_PEAK_GBS = 8000.0                   # as bench.py


def omegas(K):
    return 1.405189e-4*(1.0 + 0.07*np.arange(K))


class HostStatistics(DiagnosticCallback):
    """what a user script did before: read both fields on the host at every sampled step, update the accumulators in numpy"""
    name = 'hoststats'

    def __init__(self, solver_obj, om, every):
        super(HostStatistics, self).__init__(solver_obj, append_to_log=False)
        self.om, self.every, self.acc = om, every, None

    def evaluate(self, index=None):
        s = self.solver_obj
        if s.iteration % self.every:
            return
        eta = s.fields.elev_2d.dat.data_ro
        uv = s.fields.uv_2d.dat.data_ro
        if self.acc is None:
            self.acc = HostFieldStats(eta.shape, len(self.om))
        self.acc.append(uv, eta, harmonic_weights(self.om, s.simulation_time))


def make_solver(nx, ny):
    lx, ly = 100e3, 100e3*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    P1 = get_functionspace(mesh, 'CG', 1)
    bath = Function(P1).interpolate(lambda x, y: 20.0 - 10.0*x/lx)
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    o.timestep = 0.05*(lx/nx)/np.sqrt(9.81*20.0)
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.output_directory = os.path.join('outputs', 'statsbench')
    s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.1)}}
    s.assign_initial_conditions(elev=Constant(0.0))
    s.print_state = lambda *a, **k: None
    return s


def run(nx, ny, steps, case, K, warmup, repeats):
    s = make_solver(nx, ny)
    o = s.options
    every = 10 if case.endswith('10') else 1
    if case.startswith('b'):
        s.add_callback(FieldStatisticsCallback(s, harmonics={'c{:d}'.format(k): w for k, w in enumerate(omegas(K))}, every=every,
                                               export_to_hdf5=False), eval_interval='timestep')
    elif case.startswith('c'):
        s.add_callback(HostStatistics(s, omegas(K), every), eval_interval='timestep')

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
    s.timestepper.device.close()
    return out


def kernel_alone(nx, ny, K, appends, repeats):
    """(ms per append, GB/s on the kernel's byte model) of ``appends`` back-to-back launches between two synchronisations"""
    s = make_solver(nx, ny)
    dev = s.timestepper.device
    dev.advance(1)
    sid = dev.stats_create(K)
    w = harmonic_weights(omegas(K), 1000.0)

    def burst(n):
        dev.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            dev.stats_append(sid, w)
        dev.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    burst(10)
    ms = float(np.median([burst(appends) for _ in range(repeats)]))
    nodes = dev.n_cells*dev.npc
    gbs = nodes*(24.0 + 16.0*(8 + 2*K))/(ms*1e-3)/1e9
    dev.close()
    return ms, gbs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--constituents', type=int, default=8)
    ap.add_argument('--cases', default='a,b1,b10,c1,c10')
    args = ap.parse_args()
    K = args.constituents
    res = {'cells': 2*args.nx*args.ny, 'steps': args.steps, 'repeats': args.repeats, 'constituents': K}
    for c in args.cases.split(','):
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.steps, c, K, args.warmup, args.repeats)
    ms, gbs = kernel_alone(args.nx, args.ny, K, 100, args.repeats)
    res.update({'kernel_ms_per_append': ms, 'kernel_model_bytes_per_cell': 3*(24 + 16*(8 + 2*K)), 'kernel_gbs': gbs,
                'kernel_frac_of_peak': gbs/HBM_PEAK_GBS})
    if 'ms_per_step_b1' in res and 'ms_per_step_c1' in res:
        res['c1_over_b1'] = res['ms_per_step_c1']/res['ms_per_step_b1']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
