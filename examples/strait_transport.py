#!/usr/bin/env python
"""
Tidal prism of a basin behind a strait: a channel whose open end (boundary 1, x = 0) follows an M2-like tide, narrowed to a throat
half way along and closed at the far end.  A ``SectionTransportCallback`` sums - on the device, every fifth step, without leaving the
batched ``iterate()`` - the volume transport through a transect across the throat and through the open boundary, and the flux of a
tracer through both.  The transect is walked from the south bank to the north bank, so its right-hand normal points into the basin:
flood is positive there; the boundary section counts along the outward normal: flood is negative there.  The tidal prism is the range
of the cumulative volume.

    python examples/strait_transport.py [--nx 32 --ny 8 --periods 2 --period 44714 --every 5 --step-loop]
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thetis_amd import (Constant, Function, HarmonicTidalForcing, Mesh2d, RectangleMesh, SectionTransportCallback,   # noqa: E402
                        get_functionspace, solver2d)

LX, LY, DEPTH = 20e3, 4e3, 20.0


def strait_mesh(nx, ny):
    """the rectangle's triangles with the banks drawn in to half the width around x = LX/2; marker 1: the open end, 2: the rest"""
    rect = RectangleMesh(nx, ny, LX, LY)
    xy = np.array(rect.vertex_xy)
    squeeze = 1.0 - 0.5*np.exp(-((xy[:, 0] - 0.5*LX)/(0.1*LX))**2)
    xy[:, 1] = 0.5*LY + (xy[:, 1] - 0.5*LY)*squeeze
    return Mesh2d(xy, rect.cells, marker_fn=lambda xm, ym: np.where(np.abs(xm) < 1e-6, 1, 2))


def setup(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=32)
    ap.add_argument('--ny', type=int, default=8)
    ap.add_argument('--periods', type=float, default=2.0, help='length of the run in tidal periods')
    ap.add_argument('--period', type=float, default=12.4206012*3600.0, help='tidal period, seconds')
    ap.add_argument('--every', type=int, default=5, help='sample every n-th step')
    ap.add_argument('--step-loop', action='store_true', help='take the time loop step by step instead of in batches')
    args = ap.parse_args(argv)
    mesh2d = strait_mesh(args.nx, args.ny)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').interpolate(lambda x, y: DEPTH - 5.0*x/LX)

    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    options = solver_obj.options
    dmin = min(LX/args.nx, 0.5*LY/args.ny)
    options.timestep = 0.1*dmin/math.sqrt(9.81*DEPTH)          # explicit, inside the gravity-wave limit of the throat's triangles
    n_steps = int(math.ceil(args.periods*args.period/options.timestep))
    options.simulation_export_time = max(n_steps//8, 1)*options.timestep
    options.simulation_end_time = (n_steps - 0.5)*options.timestep
    options.swe_timestepper_type = 'SSPRK33'
    options.swe_timestepper_options.use_automatic_timestep = False
    options.no_exports = True
    options.quadratic_drag_coefficient = Constant(0.0025)
    options.add_tracer_2d('salt_2d', 'Depth averaged salinity', 'Salinity2d', source=None, diffusivity=None)
    options.tracer_timestepper_type = 'SSPRK33'
    options.tracer_timestepper_options.use_automatic_timestep = False

    y = P1_2d.node_xy()[:, 1]
    omega = 2*math.pi/args.period
    tide = HarmonicTidalForcing(Function(P1_2d, name='tidal_elev'), [omega], np.stack([0.5 + 0.0*y]), np.stack([0.5*math.pi + 0.0*y]),
                                mean=0.0)                      # 0.5 sin(omega t): the run starts at rest, on the rising tide
    solver_obj.bnd_functions['shallow_water'] = {1: {'elev': tide}}
    solver_obj.bnd_functions['salt_2d'] = {1: {'value': Constant(35.0)}}
    solver_obj.assign_initial_conditions(elev=Constant(0.0), salt_2d=Function(P1_2d).interpolate(lambda x, y: 35.0 - 10.0*x/LX))
    sections = SectionTransportCallback(solver_obj, {'throat': [(0.5*LX, -1.0), (0.5*LX, LY + 1.0)], 'open': 1}, tracers=('salt_2d',),
                                        every=args.every, append_to_log=False, export_to_hdf5=False)
    solver_obj.add_callback(sections, 'timestep')
    return solver_obj, sections, args


def main(argv=None):
    solver_obj, sections, args = setup(argv)
    if args.step_loop:
        for _ in solver_obj.create_iterator():
            pass
    else:
        solver_obj.iterate()
    r = sections.result()
    print('steps {:d}  samples {:d}  section lengths {:.1f} m (throat), {:.1f} m (open boundary)'.format(
        solver_obj.iteration, len(r['time']), r['length'][0], r['length'][1]))
    for j, name in enumerate(sections.section_names):
        q, cum = r['transport'][:, j], r['cumulative_volume'][:, j]
        print('{:6s} transport {:+.6e} ... {:+.6e} m3/s   mean depth-averaged normal velocity up to {:.4f} m/s   '
              'tidal prism {:.6e} m3   salt flux {:+.6e} ... {:+.6e}'.format(
                  name, q.min(), q.max(), np.abs(q/r['area'][:, j]).max(), cum.max() - cum.min(),
                  r['tracer_transport'][:, j, 0].min(), r['tracer_transport'][:, j, 0].max()))
    return solver_obj, sections


if __name__ == '__main__':
    main()
