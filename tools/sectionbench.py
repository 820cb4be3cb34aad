"""ms per time step of FlowSolver2d.iterate with section transports (thetis_amd/sections.py, csrc/swe2d_sections.hip) on the bench
channel:
(a)       no callback;
(d1_1)    SectionTransportCallback on the device, 1 section, every = 1;      (d1_10)   the same with every = 10;
(d16_1)   16 sections, every = 1;                                            (d16_10)  every = 10;
(h1_1)    a host callback that reads uv_2d and elev_2d at every sampled step and integrates the same pieces in numpy, 1 section,
          every = 1;      (h1_10)  every = 10;      (h16_1), (h16_10)  16 sections;
and the section kernel alone: ms per appended row in a burst of launches between two synchronisations, for 1 and for 16 sections.

    python tools/sectionbench.py [--nx 707 --ny 707] [--steps 200] [--pieces 1000]

RectangleMesh(nx, ny) has 2*nx*ny triangles: 707 x 707 is the bench mesh (1 M), 250 x 250 a dataflow-size mesh (125 k).  A section is
an oblique line long enough to be cut into about ``--pieces`` pieces; the 16 sections are such lines side by side.  The pieces are
cut once and handed to every case.  Each case is timed ``--repeats`` times in the same process; the median is reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from thetis_amd import Constant, Function, RectangleMesh, SectionTransportCallback, get_functionspace, sections, solver2d  # noqa: E402
from thetis_amd.callback import DiagnosticCallback  # noqa: E402

LX = 100e3


class HostTransport(DiagnosticCallback):
    """what a user script did before: read both fields on the host at every sampled step, integrate along the pieces in numpy"""
    name = 'hosttransport'

    def __init__(self, solver_obj, pieces, every):
        super(HostTransport, self).__init__(solver_obj, append_to_log=False)
        self.pieces, self.every, self.rows = pieces, every, []
        self.h = solver_obj.fields.bathymetry_2d.cell_node_values()

    def evaluate(self, index=None):
        s = self.solver_obj
        if s.iteration % self.every:
            return
        uv = s.fields.uv_2d.cell_node_values()
        eta = s.fields.elev_2d.cell_node_values()
        row = []
        for p in self.pieces:
            c, w = p.cell, p.weights
            H = np.einsum('pqi,pi->pq', w, eta[c] + self.h[c])
            un = np.einsum('pqi,pi->pq', w, uv[c, :, 0])*p.normal[:, :1] + np.einsum('pqi,pi->pq', w, uv[c, :, 1])*p.normal[:, 1:]
            row.append((float(np.sum(H*un)), float(np.sum(0.5*p.length[:, None]*H))))
        self.rows.append(row)


def make_solver(nx, ny):
    lx, ly = LX, LX*ny/nx
    mesh = RectangleMesh(nx, ny, lx, ly)
    P1 = get_functionspace(mesh, 'CG', 1)
    bath = Function(P1).interpolate(lambda x, y: 20.0 - 10.0*x/lx)
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    o.timestep = 0.05*(lx/nx)/np.sqrt(9.81*20.0)
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    o.output_directory = os.path.join('outputs', 'sectionbench')
    s.bnd_functions['shallow_water'] = {1: {'elev': Constant(0.1)}}
    s.assign_initial_conditions(elev=Constant(0.0))
    s.print_state = lambda *a, **k: None
    return s


def cut_sections(mesh, nx, ny, n_pieces):
    """16 oblique lines side by side, each cut into about ``n_pieces`` pieces (a line that rises one cell in four crosses about 2.5
    edges per column of the grid)"""
    ly = LX*ny/nx
    span = min(0.9, n_pieces/(2.5*nx))*LX
    out = []
    for j in range(16):
        y0 = (0.05 + 0.04*j)*ly
        out.append(sections.cut_polyline(mesh, [(0.03*LX, y0), (0.03*LX + span, y0 + 0.25*span*ly/LX)]))
    return out


def run(nx, ny, steps, case, pieces, warmup, repeats):
    s = make_solver(nx, ny)
    o = s.options
    if case != 'a':
        kind, every = case.split('_')
        chosen = pieces[:int(kind[1:])]
        every = int(every)
        if kind[0] == 'd':
            cb = SectionTransportCallback(s, {'s{:d}'.format(j): p for j, p in enumerate(chosen)}, every=every, append_to_log=False,
                                          export_to_hdf5=False)
        else:
            cb = HostTransport(s, chosen, every)
        s.add_callback(cb, eval_interval='timestep')

    def batch(n):
        o.simulation_export_time = n*o.timestep
        o.simulation_end_time = s.simulation_time + (n - 0.5)*o.timestep
        s.export_initial_state = False
        t0 = time.perf_counter()
        s.iterate()
        if case.startswith('d'):
            cb.result()                           # the rows of the batch are read inside the timed span
        s.timestepper.device.synchronize()
        return 1e3*(time.perf_counter() - t0)/n
    batch(warmup)
    out = float(np.median([batch(steps) for _ in range(repeats)]))
    s.timestepper.device.close()
    return out


def kernel_alone(nx, ny, pieces, appends, repeats):
    """ms per appended row of ``appends`` back-to-back launches between two synchronisations, for 1 and for 16 sections"""
    s = make_solver(nx, ny)
    dev = s.timestepper.device
    dev.advance(1)
    out = {}
    for n in (1, 16):
        chosen = pieces[:n]
        dev.sections_set(n, np.concatenate([np.full(len(p), j) for j, p in enumerate(chosen)]), np.concatenate([p.cell for p in chosen]),
                         np.concatenate([p.weights for p in chosen]), np.concatenate([p.normal for p in chosen]))

        def burst(m):
            dev.sections_rows_reserve(m)
            dev.synchronize()
            t0 = time.perf_counter()
            for _ in range(m):
                dev.sections_rows_append()
            dev.synchronize()
            ms = 1e3*(time.perf_counter() - t0)/m
            dev.sections_rows_read()
            return ms
        burst(10)
        out['kernel_ms_per_row_{:d}'.format(n)] = float(np.median([burst(appends) for _ in range(repeats)]))
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=707)
    ap.add_argument('--ny', type=int, default=707)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--pieces', type=int, default=1000)
    ap.add_argument('--cases', default='a,d1_1,d1_10,d16_1,d16_10,h1_1,h1_10,h16_1,h16_10')
    ap.add_argument('--no-kernel', action='store_true', help='skip the bursts of the kernel alone (needs a device with section calls)')
    args = ap.parse_args()
    mesh = make_solver(args.nx, args.ny)
    pieces = cut_sections(mesh.mesh2d, args.nx, args.ny, args.pieces)
    mesh.timestepper.device.close()
    res = {'cells': 2*args.nx*args.ny, 'steps': args.steps, 'repeats': args.repeats,
           'pieces_per_section': [len(p) for p in pieces][:2] + ['...'], 'pieces_16_sections': int(sum(len(p) for p in pieces))}
    for c in args.cases.split(','):
        res['ms_per_step_' + c] = run(args.nx, args.ny, args.steps, c, pieces, args.warmup, args.repeats)
    if not args.no_kernel:
        res.update(kernel_alone(args.nx, args.ny, pieces, 100, args.repeats))
    for n in (1, 16):
        d, h = res.get('ms_per_step_d{:d}_1'.format(n)), res.get('ms_per_step_h{:d}_1'.format(n))
        if d and h:
            res['h{0:d}_1_over_d{0:d}_1'.format(n)] = h/d
    print(json.dumps(res))


if __name__ == '__main__':
    main()
