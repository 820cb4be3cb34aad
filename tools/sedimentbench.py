"""ms per coupled time step of FlowSolver2d.iterate - flow, one P1DG field, limiter, SSPRK33 - on a flat channel
(thetis_amd/sediment_model.py, csrc/swe2d_sediment.hip):
(a)  a plain tracer in place of the sediment (what the same run cost before the sediment passes existed);
(b)  suspended sediment + Exner on the device: the coefficient and facet kernels once per step, the source kernel in front of each of
     the three sediment stages, the Exner kernel and the copy of the bed; batched by swe2d_advance_coupled;
(c)  the same through the host fallback: a device class without ``sediment_set`` - per step the stepper pulls the flow, evaluates
     ``HostSediment`` in numpy, pulls the field and uploads the source per stage, and uploads the new bed;
(d)  as (b) with ``use_bedload`` and the default slope corrections, the bedload pass as a launch of its own after the limiter
     (``fuse_with_sediment = 0``): one more kernel per step (swe_bedload_kernel) and the gather of its contribution planes in the Exner
     kernel;
(e)  as (d) with q_b evaluated in the coefficient pass's launch (``fuse_with_sediment``, what FlowSolver2d takes): one launch fewer
     per step, the friction closures once per node for both - the same bits;
(f)  as (e) with ``use_sediment_slide`` (length scale 0.2, 22 degrees): one more kernel per step (swe_slide_kernel) in front of the
     Exner kernel, a 8-byte clear of its maximum word, and the gather of its contribution planes as a third sum.

    python tools/sedimentbench.py [--nx 707 --ny 707] [--steps 100] [--host-steps 3]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  All cases
of a mesh run in the same process, one after the other, each ``--repeats`` times; the median is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, Function, RectangleMesh, get_functionspace, solver2d  # noqa: E402
from thetis_amd.device import Swe2dDevice  # noqa: E402


class HostFallbackDevice(Swe2dDevice):
    """the device without the sediment calls: the stepper takes the per-stage host evaluation"""

    @property
    def sediment_set(self):
        raise AttributeError('sediment_set')


def make_solver(nx, ny, case):
    lx, ly = 1600.0, 1600.0*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    s = solver2d.FlowSolver2d(mesh, Function(get_functionspace(mesh, 'CG', 1), name='bathymetry_2d').assign(0.4))
    if case == 'c':
        s._device_cls = HostFallbackDevice
    o, so = s.options, s.options.sediment_model_options
    o.no_exports = True
    o.output_directory = os.path.join('outputs', 'sedimentbench')
    if case != 'a':
        so.solve_suspended_sediment = True
        so.solve_exner = True
        so.use_advective_velocity_correction = False
        so.average_sediment_size = Constant(160e-6)
        so.bed_reference_height = Constant(0.025)
        so.morphological_viscosity = Constant(1e-6)
        so.morphological_acceleration_factor = Constant(100.0)
        so.use_bedload = case in ('d', 'e', 'f')
        if case == 'f':
            so.use_sediment_slide = True
            so.sed_slide_length_scale = Constant(0.2)
            so.max_angle = Constant(22)
        if case in ('d', 'e', 'f'):
            from thetis_amd.sediment_model import SedimentModel
            so.sediment_model_class = type('BenchSedimentModel', (SedimentModel,), {'fuse_bedload': case in ('e', 'f')})
    o.set_timestepper_type('SSPRK33')
    for t in (o.swe_timestepper_options, o.tracer_timestepper_options, so.sediment_timestepper_options):
        if hasattr(t, 'use_automatic_timestep'):
            t.use_automatic_timestep = False
    o.timestep = 0.05*(lx/nx)/2.5                       # a twentieth of the gravity-wave limit
    uv = lambda x, y: (0.5 + 0.05*np.sin(6.28*x/lx), 0.0*x)      # noqa: E731
    if case == 'a':
        c = Function(get_functionspace(mesh, 'DG', 1), name='c_2d')
        o.add_tracer_2d('c_2d', 'Tracer', 'Tracer2d', function=c)
        s.assign_initial_conditions(uv=uv, c=Function(c.function_space()).assign(1.0))
    else:
        s.assign_initial_conditions(uv=uv)
        assert s.timestepper.tracers['sediment_2d'].host_sediment == (case == 'c')
    s.print_state = lambda *a, **k: None
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
    field = s.fields['c_2d' if case == 'a' else 'sediment_2d']
    assert np.isfinite(field.dat.data_ro).all()
    if case != 'a':
        assert np.isfinite(s.fields.bathymetry_2d.dat.data_ro).all()
    s.timestepper.device.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--host-steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='a,b,c,d,e,f')
    args = ap.parse_args()
    res = {'cells': 2*args.nx*args.ny, 'steps': args.steps, 'host_steps': args.host_steps, 'repeats': args.repeats}
    for c in args.cases.split(','):
        host = c == 'c'
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.host_steps if host else args.steps, c,
                                      1 if host else args.warmup, 1 if host else args.repeats)
    if 'ms_per_step_a' in res and 'ms_per_step_b' in res:
        res['b_minus_a_ms_per_step'] = res['ms_per_step_b'] - res['ms_per_step_a']
    if 'ms_per_step_b' in res and 'ms_per_step_d' in res:
        res['d_minus_b_ms_per_step'] = res['ms_per_step_d'] - res['ms_per_step_b']
    if 'ms_per_step_d' in res and 'ms_per_step_e' in res:
        res['e_minus_d_ms_per_step'] = res['ms_per_step_e'] - res['ms_per_step_d']
    if 'ms_per_step_e' in res and 'ms_per_step_f' in res:
        res['f_minus_e_ms_per_step'] = res['ms_per_step_f'] - res['ms_per_step_e']
    if 'ms_per_step_b' in res and 'ms_per_step_c' in res:
        res['c_over_b'] = res['ms_per_step_c']/res['ms_per_step_b']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
