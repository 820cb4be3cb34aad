"""
Detector scenarios shared by tests/test_detectors.py (CPU, host stand-in device) and tests/test_gpu_detectors.py (HIP library):
a FlowSolver2d user script with per-time-step and per-export detectors, run on one rank or partitioned over several
(``run_detectors``: a spawn target of its own, the pattern of tests/dist_worker.py).
"""
import os

import numpy as np

from cpu_device import CpuSwe2dDevice
from thetis_amd import pointeval


class CpuProbeDevice(CpuSwe2dDevice):
    """The host stand-in with the probe entry points: the weighted sum of thetis_amd/pointeval.py on the stand-in's state."""

    def __init__(self, *args, **kwargs):
        super(CpuProbeDevice, self).__init__(*args, **kwargs)
        self._probes = {}
        self._next_probe = 0

    def _probe_values(self, cells, weights, fields):
        uv, eta = self.get_state()
        cols = []
        for f in fields:
            if f == 'uv':
                cols.append(pointeval.evaluate(uv, cells, weights))
            elif f == 'elev':
                cols.append(pointeval.evaluate(eta, cells, weights)[:, None])
            else:
                cols.append(pointeval.evaluate(self.tracer_get_state(f), cells, weights)[:, None])
        return np.hstack(cols)

    def probe_create(self, cells, weights, fields, capacity=0):
        pid = self._next_probe
        self._next_probe += 1
        self._probes[pid] = dict(cells=np.asarray(cells), weights=np.asarray(weights), fields=list(fields), capacity=int(capacity), rows=[])
        return pid

    def probe_append(self, pid):
        p = self._probes[pid]
        assert len(p['rows']) < p['capacity']
        p['rows'].append(self._probe_values(p['cells'], p['weights'], p['fields']))

    def probe_read(self, pid):
        p = self._probes[pid]
        rows, p['rows'] = p['rows'], []
        return np.array(rows)

    def probe_eval(self, pid):
        p = self._probes[pid]
        return self._probe_values(p['cells'], p['weights'], p['fields'])

    def probe_destroy(self, pid):
        del self._probes[pid]


def channel_with_detectors(outdir, nx=24, ny=4, tracer=False, end_time=400.0):
    """a closed channel with a dam-break initial state; detectors every step ('gauges') and at every export ('probes')"""
    from thetis_amd import DetectorsCallback, Function, RectangleMesh, get_functionspace, solver2d
    lx, ly = 100e3, 4000.0
    mesh2d = RectangleMesh(nx, ny, lx, ly)
    P1_2d = get_functionspace(mesh2d, 'CG', 1)
    bathymetry_2d = Function(P1_2d, name='Bathymetry').interpolate(lambda x, y: 20.0 + (5.0 - 20.0)*x/lx)
    solver_obj = solver2d.FlowSolver2d(mesh2d, bathymetry_2d)
    o = solver_obj.options
    o.simulation_export_time = 100.0
    o.simulation_end_time = end_time
    o.timestep = 5.0
    o.output_directory = outdir
    o.no_exports = True
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    if tracer:
        o.add_tracer_2d('tracer_2d', 'Depth averaged tracer', 'Tracer2d')
    solver_obj.create_equations()
    xy = [(1.3e3 + 4.1e3*i, 0.37*ly + 50.0*i) for i in range(20)] + [(lx/nx, ly/ny)]    # the last one on a vertex
    fields = ['elev_2d', 'uv_2d'] + (['tracer_2d'] if tracer else [])
    solver_obj.add_callback(DetectorsCallback(solver_obj, xy, fields, 'gauges'), 'timestep')
    solver_obj.add_callback(DetectorsCallback(solver_obj, xy[::-1], ['uv_2d'], 'probes'), 'export')
    elev_init = Function(P1_2d).interpolate(lambda x, y: np.where(x < 30e3, 6.0*(1 - x/30e3), 0.0))
    kw = {'tracer_2d': Function(P1_2d).interpolate(lambda x, y: np.exp(-((x - 50e3)/10e3)**2))} if tracer else {}
    solver_obj.assign_initial_conditions(elev=elev_init, **kw)
    solver_obj.iterate()
    return solver_obj


def result(solver_obj, outdir):
    out = {}
    for mode in ('timestep', 'export'):
        for name, cb in solver_obj.callbacks[mode].items():
            if hasattr(cb, 'detector_names'):
                out[name] = ([h[0] for h in cb.history], np.array([h[1] for h in cb.history]))
    solver_obj.comm.barrier()
    for f in sorted(os.listdir(outdir)):
        if f.endswith('.npz'):
            with np.load(os.path.join(outdir, f)) as z:
                out[f] = {k: z[k] for k in z.files}
    return out


def detector_worker(rank, world, port, out_dir, cpu, tracer):
    import pickle
    os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'RANK': str(rank), 'WORLD_SIZE': str(world),
                       'LOCAL_RANK': str(rank), 'LOCAL_WORLD_SIZE': str(world), 'THETIS_AMD_DIST_BACKEND': 'gloo'})
    from thetis_amd import solver2d
    if cpu:
        solver2d.FlowSolver2d._device_cls = CpuProbeDevice
    outdir = os.path.join(out_dir, 'out_w{:d}'.format(world))
    res = result(channel_with_detectors(outdir, tracer=tracer), outdir)
    with open(os.path.join(out_dir, 'det_w{:d}_r{:d}.pkl'.format(world, rank)), 'wb') as f:
        pickle.dump(res, f)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def run_detectors(world, out_dir, cpu=True, tracer=False, timeout=600):
    """spawn ``world`` ranks of ``detector_worker``; the per-rank results"""
    import multiprocessing as mp
    import pickle
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=detector_worker, args=(r, world, port, out_dir, cpu, tracer)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    for p in procs:
        if p.is_alive():
            for q in procs:
                if q.is_alive():
                    q.terminate()
            raise RuntimeError('detector worker timed out')
        assert p.exitcode == 0, 'detector worker failed with exit code {:}'.format(p.exitcode)
    out = []
    for r in range(world):
        with open(os.path.join(out_dir, 'det_w{:d}_r{:d}.pkl'.format(world, r)), 'rb') as f:
            out.append(pickle.load(f))
    return out


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], dict):
            assert sorted(a[k]) == sorted(b[k]), k
            for kk in a[k]:
                assert np.array_equal(a[k][kk], b[k][kk]), (k, kk)
        else:
            assert a[k][0] == b[k][0], k
            assert np.array_equal(a[k][1], b[k][1]), k
