#!/usr/bin/env python
"""
Gray-Scott reaction-diffusion: two tracers that diffuse at different rates and feed on each other,

    da/dt = D1 lap a + gamma (1 - a) - a b^2,        db/dt = D2 lap b + a b^2 - (gamma + kappa) b,

the test case of Hundsdorfer & Verwer (2003), "Numerical Solution of Time-Dependent Advection-Diffusion-Reaction Equations".  The
sources are written as expressions of the two tracer Functions; the device evaluates them in front of every stage from the current
tracer values (``thetis_amd.reactions``) and ``iterate()`` keeps its batches.

Set-up: a closed square box of side 2.5 (walls without a boundary dict are zero-flux), triangles, P1DG tracers, no flow
(``tracer_only``), SSPRK33, SIPG diffusion with D1 = 8e-5 and D2 = 4e-5, gamma = 0.024, kappa = 0.06; a = 1 - 2 b and a patch of b
in the middle.  The time step is explicit: the SIPG operator limits it to about h^2/(C D1) with C of the order of the penalty (tens for
P1), the kinetics to 1/(gamma + kappa + b^2) ~ 1; the script takes dt = min(0.01 h^2/D1, 0.5) with h the shortest edge - 0.31 on the
default 50 x 50 mesh, a small fraction of the diffusive limit, and never more than half the kinetic one.

    python examples/gray_scott.py [--n 50 --end 200 --no-diffusion --outdir outputs]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (And, Constant, Function, SquareMesh, SpatialCoordinate, conditional, get_functionspace, pi, sin,     # noqa: E402
                        solver2d)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50, help='cells per side')
    ap.add_argument('--end', type=float, default=200.0, help='simulation end time')
    ap.add_argument('--no-diffusion', action='store_true', help='kinetics only')
    ap.add_argument('--outdir', default='outputs')
    args = ap.parse_args(argv)
    side = 2.5
    mesh2d = SquareMesh(args.n, args.n, side)
    x, y = SpatialCoordinate(mesh2d)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    P1DG_2d = get_functionspace(mesh2d, 'DG', 1)
    bathymetry2d = Function(P1_2d).assign(1.0)

    D1, D2 = Constant(8.0e-05), Constant(4.0e-05)
    gamma, kappa = Constant(0.024), Constant(0.06)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry2d)
    options = solver_obj.options
    options.tracer_only = True
    options.use_limiter_for_tracers = False
    options.no_exports = True
    options.output_directory = args.outdir
    options.set_timestepper_type('SSPRK33')
    options.tracer_timestepper_options.use_automatic_timestep = False
    options.swe_timestepper_options.use_automatic_timestep = False
    h = side/args.n
    dt = min(0.01*h*h/float(D1), 0.5)
    options.timestep = dt
    n_steps = max(1, int(round(args.end/dt)))
    options.simulation_end_time = n_steps*dt
    options.simulation_export_time = max(1, n_steps//4)*dt

    a_2d, b_2d = Function(P1DG_2d, name='a_2d'), Function(P1DG_2d, name='b_2d')
    options.add_tracer_2d('a_2d', 'Tracer A', 'TracerA2d', function=a_2d, diffusivity=None if args.no_diffusion else D1,
                          source=gamma - a_2d*b_2d**2 - gamma*a_2d)
    options.add_tracer_2d('b_2d', 'Tracer B', 'TracerB2d', function=b_2d, diffusivity=None if args.no_diffusion else D2,
                          source=a_2d*b_2d**2 - (gamma + kappa)*b_2d)

    tracer_b_init = Function(P1DG_2d).interpolate(
        conditional(And(And(1.0 <= x, x <= 1.5), And(1.0 <= y, y <= 1.5)), 0.25*sin(4*pi*x)**2*sin(4*pi*y)**2, 0.0))
    tracer_a_init = Function(P1DG_2d).interpolate(1.0 - 2.0*tracer_b_init)
    solver_obj.assign_initial_conditions(a=tracer_a_init, b=tracer_b_init)
    solver_obj.iterate()

    a, b = solver_obj.fields.a_2d.dat.data_ro, solver_obj.fields.b_2d.dat.data_ro
    print('steps {:d}  dt {:.4f}  t {:.2f}'.format(solver_obj.iteration, dt, solver_obj.simulation_time))
    print('a {:.6f} ... {:.6f}   b {:.6f} ... {:.6f}'.format(a.min(), a.max(), b.min(), b.max()))
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return solver_obj


if __name__ == '__main__':
    main()
