"""ms per time step of FlowSolver2d.iterate with a tidal elevation on the open end of a channel (thetis_amd/forcing.py,
csrc/swe2d_tide.hip):
(a) a constant elevation, the handle kept on stage launches (SWE2D_OPT_FUSED_STAGES = 0, SWE2D_OPT_FLOW = 0): what (b) adds its
    three tide launches per step to;
(b) the M2 + S2 tide evaluated on the device, the steps batched;
(c) the same tide through ``update_forcings`` + ``set_tidal_field``: Python, one compact upload and one stage launch per stage.

    python tools/tidebench.py [--nx 707 --ny 707] [--steps 200]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  Each case
is timed ``--repeats`` times in the same process, one after the other; the median is reported."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, Function, HarmonicTidalForcing, RectangleMesh, _lib, get_functionspace, solver2d  # noqa: E402


def run(nx, ny, steps, case, warmup, repeats):
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
    o.output_directory = os.path.join('outputs', 'tidebench')
    y = P1.node_xy()[:, 1]
    tide = HarmonicTidalForcing(Function(P1), [2*math.pi/(12.4206012*3600.0), 2*math.pi/(12.0*3600.0)],
                                np.stack([0.8*(1.0 + 0.1*y/ly), 0.3*(1.0 + 0.1*y/ly)]), np.stack([0.2*y/ly, 0.7 + 0.2*y/ly]))
    elev = {'a': Constant(0.1), 'b': tide, 'c': tide.elev_field}[case]
    s.bnd_functions['shallow_water'] = {1: {'elev': elev}}
    s.assign_initial_conditions(elev=Constant(0.0))
    if case == 'a':
        s.timestepper.device.set_option(_lib.OPT_FUSED_STAGES, 0)
        s.timestepper.device.set_option(_lib.OPT_FLOW, 0)
    forcings = (lambda t: tide.set_tidal_field(t)) if case == 'c' else None
    s.print_state = lambda *a, **k: None

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='abc')
    args = ap.parse_args()
    res = {'cells': 2*args.nx*args.ny, 'steps': args.steps, 'repeats': args.repeats}
    for c in args.cases:
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.steps, c, args.warmup, args.repeats)
    if 'ms_per_step_a' in res and 'ms_per_step_b' in res:
        res['b_over_a'] = res['ms_per_step_b']/res['ms_per_step_a']
    if 'ms_per_step_b' in res and 'ms_per_step_c' in res:
        res['c_over_b'] = res['ms_per_step_c']/res['ms_per_step_b']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
