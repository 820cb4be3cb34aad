"""ms per time step of FlowSolver2d.iterate with gauges sampled at every step (DetectorsCallback, csrc/swe2d_probe.hip):
(a) no detectors, (b) 100 per-time-step detectors on the device path (the steps stay batched, a row is appended after every step),
(c) the same 100 points read through get_state at every step (the only way before: the whole state to the host).

    python tools/detectorbench.py [--nx 707 --ny 707] [--steps 200] [--points 100]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import DetectorsCallback, Function, RectangleMesh, get_functionspace, solver2d  # noqa: E402
from thetis_amd.callback import DiagnosticCallback  # noqa: E402
from thetis_amd.pointeval import PointLocator, evaluate  # noqa: E402


class HostGauges(DiagnosticCallback):
    """case (c): the points evaluated on a host copy of the whole state"""
    name = 'host_gauges'

    def __init__(self, solver_obj, xy):
        super(HostGauges, self).__init__(solver_obj, append_to_log=False)
        self.loc = PointLocator(solver_obj.mesh2d, xy)

    def __call__(self):
        uv, eta = self.solver_obj.timestepper.device.get_state()
        return np.hstack([evaluate(eta, self.loc.cells, self.loc.weights)[:, None], evaluate(uv, self.loc.cells, self.loc.weights)])

    def evaluate(self, index=None):
        self.history.append((self.solver_obj.simulation_time, self()))


def run(nx, ny, steps, points, case, warmup):
    lx, ly = 100e3, 100e3*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    bath = Function(get_functionspace(mesh, 'CG', 1)).interpolate(lambda x, y: 20.0 - 10.0*x/lx)
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    dx = lx/nx
    o.timestep = 0.05*dx/np.sqrt(9.81*20.0)
    o.simulation_export_time = (steps + warmup)*o.timestep
    o.simulation_end_time = (steps + warmup - 0.5)*o.timestep
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.output_directory = os.path.join('outputs', 'detectorbench')
    s.create_equations()
    xy = np.random.default_rng(0).uniform([0.02*lx, 0.02*ly], [0.98*lx, 0.98*ly], size=(points, 2))
    if case == 'b':
        s.add_callback(DetectorsCallback(s, xy, ['elev_2d', 'uv_2d'], 'gauges', export_to_hdf5=False), 'timestep')
    elif case == 'c':
        s.add_callback(HostGauges(s, xy), 'timestep')
    s.assign_initial_conditions(elev=Function(get_functionspace(mesh, 'CG', 1)).interpolate(
        lambda x, y: 0.5*np.exp(-((x - 0.5*lx)**2 + (y - 0.5*ly)**2)/(0.1*lx)**2)))
    s.print_state = lambda *a, **k: None
    # warm-up: the first batch builds the kernels' tables; then the timed batch
    o.simulation_end_time = (warmup - 0.5)*o.timestep
    o.simulation_export_time = warmup*o.timestep
    s.iterate()
    s.timestepper.device.synchronize()
    o.simulation_export_time = steps*o.timestep
    o.simulation_end_time = s.simulation_time + (steps - 0.5)*o.timestep
    s.export_initial_state = False
    t0 = time.perf_counter()
    s.iterate()
    s.timestepper.device.synchronize()
    return 1e3*(time.perf_counter() - t0)/steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--points', type=int, default=100)
    ap.add_argument('--cases', default='abc')
    args = ap.parse_args()
    res = {'cells': 2*args.nx*args.ny, 'points': args.points, 'steps': args.steps}
    for c in args.cases:
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.steps if c != 'c' else max(20, args.steps//10), args.points, c,
                                      args.warmup)
    if 'ms_per_step_a' in res and 'ms_per_step_b' in res:
        res['b_over_a'] = res['ms_per_step_b']/res['ms_per_step_a']
    if 'ms_per_step_b' in res and 'ms_per_step_c' in res:
        res['c_over_b'] = res['ms_per_step_c']/res['ms_per_step_b']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
