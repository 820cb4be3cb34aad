"""Shared builders of the tidal-forcing tests (tests/test_tide_forcing.py on the CPU, tests/test_gpu_tide.py on the GPU): the 8 x 4
two-marker meshes (marker 1: the open end x = 0, marker 2: every other side - the corner cells carry both), seeded harmonic tables,
the solver set-up, the host stand-in device with boundary values per facet, and the two-rank scenario for dist_worker / spmd_cases."""
import numpy as np

from cpu_device import CpuSwe2dDevice
from thetis_amd import Constant, Function, HarmonicTidalForcing, get_functionspace, solver2d
from thetis_amd.device import FacetValues
from thetis_amd.mesh import Mesh2d, _grid_cells, _grid_quads

LX, LY, NX, NY = 8000.0, 4000.0, 8, 4
EPS = float(np.finfo(np.float64).eps)


def tide_mesh(kind='triangles'):
    """'triangles': 8 x 4 quads cut into 64 triangles; 'quads': the 32 rectangles; 'general': 32 convex quadrilaterals that are
    no parallelograms (interior vertices moved)"""
    xs, ys = np.linspace(0.0, LX, NX + 1), np.linspace(0.0, LY, NY + 1)
    xx, yy = np.meshgrid(xs, ys, indexing='ij')
    xy = np.stack([xx.ravel(), yy.ravel()], axis=1)
    if kind == 'general':
        inner = (xy[:, 0] > 1.0) & (xy[:, 0] < LX - 1.0) & (xy[:, 1] > 1.0) & (xy[:, 1] < LY - 1.0)
        xy[:, 0] += np.where(inner, 150.0*np.sin(xy[:, 1]/700.0 + xy[:, 0]/900.0), 0.0)
        xy[:, 1] += np.where(inner, 120.0*np.cos(xy[:, 0]/600.0), 0.0)
    cells = _grid_cells(NX, NY, 'left') if kind == 'triangles' else _grid_quads(NX, NY)
    mesh = Mesh2d(xy, cells, marker_fn=lambda xm, ym: np.where(np.abs(xm) < 1e-6, 1, 2))
    assert mesh.boundary_markers == [1, 2] and mesh.affine == (kind != 'general')
    return mesh


def tide_tables(n_nodes, xy, K, seed=0):
    """omegas (K,), amplitudes / phases (K, n_nodes), mean (n_nodes,): M2, S2, N2 first, then seeded frequencies of the tidal band;
    amplitudes and phases vary along the boundary"""
    rng = np.random.default_rng(100 + seed)
    base = np.array([1.405189e-4, 1.454441e-4, 1.378797e-4])
    omegas = np.concatenate([base, rng.uniform(0.3e-4, 3e-4, size=max(K - 3, 0))])[:K]
    y = xy[:, 1]/LY
    amp = np.stack([(0.6/(k + 1))*(1.0 + 0.2*np.sin(2.0*y + k)) for k in range(K)])
    phase = np.stack([0.3*k + 0.5*y + 0.1*rng.uniform(size=n_nodes) for k in range(K)])
    mean = 0.05 + 0.02*y
    return omegas, amp, phase, mean


def make_forcing(mesh, K=3, family='CG', uniform=False, boundary_ids=None, seed=0):
    fs = get_functionspace(mesh, family, 1)
    elev = Function(fs, name='tidal_elev')
    om, amp, ph, mean = tide_tables(fs.node_count(), fs.node_xy(), K, seed)
    if uniform:                     # the same value at every node: what a per-marker constant boundary value can express
        amp, ph, mean = amp*0 + amp[:, :1], ph*0 + ph[:, :1], mean*0 + mean[0]
    return HarmonicTidalForcing(elev, om, amp, ph, mean=mean, boundary_ids=boundary_ids)


class CpuFacetDevice(CpuSwe2dDevice):
    """tests/cpu_device.py takes one constant per marker (the oracle's C restatement holds nothing else).  The host path of a
    HarmonicTidalForcing ends in the compact upload of a Function-valued boundary (``facet_node_values`` -> ``set_bc`` with
    ``FacetValues``): this subclass accepts that upload where the values are the same at every facet node of the marker and hands the
    constant on - the scenarios of tests/test_tide_forcing.py use spatially uniform tables for this reason.  It has no ``tide_set``."""

    def facet_node_values(self, marker, function_values, cells_of_vertices=None):
        cells, facets = self.boundary_facets(self._slot(marker))
        nxt = (facets + 1) % self.npc
        d = np.asarray(function_values)
        if cells_of_vertices is None:
            return FacetValues(np.stack([d[cells, facets], d[cells, nxt]], axis=1))
        cv = np.asarray(cells_of_vertices)
        return FacetValues(np.stack([d[cv[cells, facets]], d[cv[cells, nxt]]], axis=1))

    def set_bc(self, marker, funcs):
        out = {}
        for key, v in (funcs or {}).items():
            if isinstance(v, FacetValues):
                vals = np.asarray(v.values)
                assert key == 'elev' and vals.size and (vals == vals.flat[0]).all(), 'uniform facet values only'
                v = float(vals.flat[0])
            out[key] = v
        CpuSwe2dDevice.set_bc(self, marker, out)


def make_solver(mesh, elev_bc, dt=0.3, n_steps=6, n_export=None, stepper='SSPRK33', outdir=None, tracer=False, wd=False):
    """a FlowSolver2d on ``mesh`` with ``elev_bc`` as the elevation of marker 1 and a constant normal velocity on marker 2"""
    P1 = get_functionspace(mesh, 'CG', 1)
    bath = Function(P1).interpolate(lambda x, y: 12.0 - 3.0*x/LX + 0.5*np.sin(y/900.0))
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    o.swe_timestepper_type = stepper
    o.swe_timestepper_options.use_automatic_timestep = False
    o.timestep = dt
    o.simulation_export_time = (n_export or n_steps)*dt
    o.simulation_end_time = (n_steps - 0.5)*dt
    o.no_exports = True
    if outdir is not None:
        o.output_directory = outdir
    o.manning_drag_coefficient = Constant(0.02)
    if tracer:
        o.add_tracer_2d('tracer_2d', 'Depth averaged tracer', 'Tracer2d', source=None, diffusivity=None)
        o.tracer_timestepper_type = stepper
        o.tracer_timestepper_options.use_automatic_timestep = False
    o.use_wetting_and_drying = bool(wd)
    s.bnd_functions['shallow_water'] = {1: {'elev': elev_bc}, 2: {'un': Constant(0.01)}}
    kw = {'tracer': Function(P1).interpolate(lambda x, y: 1.0 + (x > 0.5*LX))} if tracer else {}
    s.assign_initial_conditions(elev=Function(P1).interpolate(lambda x, y: 0.1*np.cos(np.pi*x/LX)), **kw)
    return s


# ---- the scenario of the two-rank test: run through dist_worker.spmd_worker / spmd_cases.run under the name 'tide'
def _tide_case(outdir, cpu=False):
    mesh = tide_mesh('triangles')
    s = make_solver(mesh, make_forcing(mesh, K=3), dt=0.3, n_steps=20, n_export=10, outdir=outdir)
    s.iterate()
    return s


def tide_worker(rank, world, port, out_dir, name, cpu, env):
    import dist_worker
    import spmd_cases
    spmd_cases.CASES['tide'] = _tide_case
    dist_worker.spmd_worker(rank, world, port, out_dir, name, cpu=cpu, env=env)


def run_tide_ranks(world, out_dir, timeout=300):
    """``dist_worker.run_spmd`` for the scenario of this file: the per-rank result dictionaries of ``spmd_cases.run``"""
    import multiprocessing as mp
    import os
    import pickle
    import socket
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=tide_worker, args=(r, world, port, out_dir, 'tide', False, None)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    for p in procs:
        if p.is_alive():
            for q in procs:
                if q.is_alive():
                    q.terminate()
            raise RuntimeError('tide worker timed out')
        assert p.exitcode == 0, 'tide worker failed with exit code {:}'.format(p.exitcode)
    out = []
    for r in range(world):
        with open(os.path.join(out_dir, 'res_w{:d}_r{:d}.pkl'.format(world, r)), 'rb') as f:
            out.append(pickle.load(f))
    return out
