"""ms per time step of FlowSolver2d.iterate with Lagrangian particles (thetis_amd/particles.py, csrc/swe2d_particles.hip):
(a)   no callback;
(b1)  ParticleTrackerCallback on the device, every = 1;      (b10)  the same with every = 10;
(c1)  a host callback that reads uv_2d at every sampled step and makes the same move in numpy (HostParticles), every = 1;   (c10)  every = 10;
and the particle kernel alone: ms per advance of 100 advances back to back.  The walk is a divergent gather, not a stream: per cell
visited a lane touches 64 B (3 vertex ids, 6 coordinates, 1 neighbour code), per velocity 108 B, per advance 24 B read + 20 B
written of its own state; the figures are stated as measured, without a roofline.

    python tools/particlebench.py [--nx 707 --ny 707] [--particles 10000] [--steps 200] [--host-steps 20]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  All cases
of a mesh run in the same process, one after the other, each ``--repeats`` times; the median is reported.  The host cases take
``--host-steps`` steps per repeat (a numpy move of 10^6 particles takes seconds)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, Function, ParticleTrackerCallback, RectangleMesh, get_functionspace, solver2d  # noqa: E402
from thetis_amd.callback import DiagnosticCallback  # noqa: E402
from thetis_amd.particles import HostParticles  # noqa: E402
from thetis_amd.pointeval import PointLocator  # noqa: E402


class HostTracker(DiagnosticCallback):
    """what a user script could do before: read the velocity on the host at every sampled step, move the particles in numpy"""
    name = 'hosttracker'

    def __init__(self, solver_obj, xy, every):
        super(HostTracker, self).__init__(solver_obj, append_to_log=False)
        mesh = solver_obj.mesh2d
        self.every = every
        self.set = HostParticles(mesh.cells, mesh.vertex_xy, mesh.cell_nbr, mesh.cell_nbr_facet, xy, PointLocator(mesh, xy).cells)

    def evaluate(self, index=None):
        s = self.solver_obj
        if s.iteration % self.every:
            return
        self.set.advance(s.fields.uv_2d.cell_node_values(), self.every*s.dt, (1,))


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
    o.output_directory = os.path.join('outputs', 'particlebench')
    s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.1)}}
    s.assign_initial_conditions(elev=Constant(0.0))
    s.print_state = lambda *a, **k: None
    return s, lx, ly


def release(n, lx, ly):
    rng = np.random.default_rng(1)
    return np.stack([rng.uniform(0.02*lx, 0.98*lx, n), rng.uniform(0.02*ly, 0.98*ly, n)], axis=1)


def run(nx, ny, n_particles, steps, case, warmup, repeats):
    s, lx, ly = make_solver(nx, ny)
    o = s.options
    every = 10 if case.endswith('10') else 1
    if case.startswith('b'):
        s.add_callback(ParticleTrackerCallback(s, release(n_particles, lx, ly), every=every, record_every=10**9, open_boundaries=(1,),
                                               export_to_hdf5=False), eval_interval='timestep')
    elif case.startswith('c'):
        s.add_callback(HostTracker(s, release(n_particles, lx, ly), every), eval_interval='timestep')

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


def kernel_alone(nx, ny, n_particles, advances, repeats):
    """ms per advance of ``advances`` back-to-back launches between two synchronisations, in the velocity after 50 steps"""
    s, lx, ly = make_solver(nx, ny)
    dev = s.timestepper.device
    dev.advance(50)
    xy = release(n_particles, lx, ly)
    pid = dev.particles_create(xy, PointLocator(s.mesh2d, xy).cells)
    dt_move = 10*s.options.timestep

    def burst(n):
        dev.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            dev.particles_advance(pid, dt_move, (1,))
        dev.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    burst(10)
    ms = float(np.median([burst(advances) for _ in range(repeats)]))
    status = dev.particles_read(pid)[2]
    dev.close()
    return ms, int((status == 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--particles', type=int, default=10000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--host-steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='a,b1,b10,c1,c10')
    args = ap.parse_args()
    res = {'cells': 2*args.nx*args.ny, 'particles': args.particles, 'steps': args.steps, 'host_steps': args.host_steps,
           'repeats': args.repeats}
    for c in args.cases.split(','):
        host = c.startswith('c')
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.particles, args.host_steps if host else args.steps, c,
                                      min(args.warmup, args.host_steps) if host else args.warmup, args.repeats)
    ms, active = kernel_alone(args.nx, args.ny, args.particles, 100, args.repeats)
    res.update({'kernel_ms_per_advance': ms, 'kernel_ns_per_particle': 1e6*ms/args.particles, 'active_after': active})
    for e in ('1', '10'):
        if 'ms_per_step_b' + e in res and 'ms_per_step_c' + e in res:
            res['c{0}_over_b{0}'.format(e)] = res['ms_per_step_c' + e]/res['ms_per_step_b' + e]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
