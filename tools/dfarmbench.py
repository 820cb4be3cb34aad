"""ms per time step of FlowSolver2d.iterate with turbine farms in a channel (thetis_amd/turbines.py, csrc/swe2d_turbine.hip,
csrc/swe2d_dfarm.hip):
(a) no farm, the handle kept on stage launches (SWE2D_OPT_FUSED_STAGES = 0, SWE2D_OPT_FLOW = 0): what the farms add their cost to;
(b) one continuous farm on a marked subdomain (the term inside the stage kernels);
(c) one discrete farm of 16 turbines on the same subdomain (one pass per stage launch over the cells around the turbines).

    python tools/dfarmbench.py [--nx 707 --ny 707] [--steps 200] [--out profiles/r11a_dfarmbench.txt]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  Each case
is timed ``--repeats`` times in the same process, one after the other; the median is reported.  ``--out`` appends the result line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import (Constant, DiscreteTidalTurbineFarmOptions, Function, RectangleMesh, TidalTurbineFarmOptions, _lib,  # noqa: E402
                        get_functionspace, solver2d)


def run(nx, ny, steps, case, warmup, repeats):
    lx, ly = 100e3, 100e3*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly, cell_marker_fn=lambda x, y: np.where((abs(x - lx/2) < 0.1*lx) & (abs(y - ly/2) < 0.1*ly), 2, 0))
    P1 = get_functionspace(mesh, 'CG', 1)
    bath = Function(P1).interpolate(lambda x, y: 40.0 - 10.0*x/lx)
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    o.timestep = 0.05*(lx/nx)/np.sqrt(9.81*40.0)
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.output_directory = os.path.join('outputs', 'dfarmbench')
    if case == 'b':
        f = TidalTurbineFarmOptions()
        f.turbine_density = Constant(16.0/(0.2*lx*0.2*ly))
        o.tidal_turbine_farms[2] = [f]
    if case == 'c':
        d = DiscreteTidalTurbineFarmOptions()
        d.turbine_options.projected_diameter = 4.0*lx/nx                # a bump spans four cell widths
        d.turbine_coordinates = [[lx*(0.42 + 0.05*i), ly*(0.42 + 0.05*j)] for i in range(4) for j in range(4)]
        o.discrete_tidal_turbine_farms[2] = [d]
    s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.1)}}
    s.assign_initial_conditions(elev=Constant(0.0), uv=Constant((1.0, 0.0)))
    if case == 'a':
        s.timestepper.device.set_option(_lib.OPT_FUSED_STAGES, 0)
        s.timestepper.device.set_option(_lib.OPT_FLOW, 0)
    s.print_state = lambda *a, **k: None

    def batch(n):
        o.simulation_export_time = n*o.timestep
        o.simulation_end_time = s.simulation_time + (n - 0.5)*o.timestep
        s.export_initial_state = False
        t0 = time.perf_counter()
        s.iterate()
        s.timestepper.device.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    batch(warmup)
    res = float(np.median([batch(steps) for _ in range(repeats)]))
    n_list = len(s.timestepper.device.dfarm_density_read(0)[0]) if case == 'c' else 0
    return res, n_list


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='abc')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = {'cells': 2*args.nx*args.ny, 'steps': args.steps, 'repeats': args.repeats}
    for c in args.cases:
        res['ms_per_step_' + c], n_list = run(args.nx, args.ny, args.steps, c, args.warmup, args.repeats)
        if c == 'c':
            res['listed_cells_c'] = n_list
    for c in 'bc':
        if 'ms_per_step_a' in res and 'ms_per_step_' + c in res:
            res[c + '_over_a'] = res['ms_per_step_' + c]/res['ms_per_step_a']
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
