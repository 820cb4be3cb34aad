"""examples/bedload_trench.py through FlowSolver2d on the device, on meshes of a few hundred triangles: the trench with suspended load
and bedload and the bedload-only hump run; iterate()'s batches equal the generator taken step by step bit for bit for both; the
hump's centroid moves downstream; get_bedload_term() is what the device holds."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = ['--nx', '48', '--ny', '2']                                      # 192 triangles


def _example():
    spec = importlib.util.spec_from_file_location('bedload_trench', os.path.join(ROOT, 'examples', 'bedload_trench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fields(solver):
    f = solver.fields
    out = [f.uv_2d.dat.data_ro.copy(), f.elev_2d.dat.data_ro.copy(), f.bathymetry_2d.dat.data_ro.copy()]
    if hasattr(f, 'sediment_2d'):
        out.append(f.sediment_2d.dat.data_ro.copy())
    return out


@pytest.mark.parametrize('mode', [[], ['--bedload-only']])
def test_iterate_batches_equal_the_step_by_step_loop(mode):
    """12 steps in batches of 3 (iterate) against the generator taken step by step: flow, bed (and sediment) bit for bit; the
    model's bedload term is the device's planes"""
    mod = _example()
    res = []
    for batched in (True, False):
        solver, bed0, args = mod.setup(mode + MESH + ['--steps', '12'])
        model = solver.sediment_model
        assert model.on_device and model.use_bedload and sorted(model.open_markers()) == [1, 2]
        assert hasattr(solver.fields, 'sediment_2d') == (not mode)
        qbx, qby = model.get_bedload_term()                                  # of the initial flow
        assert np.isfinite(qbx).all() and qbx.max() > 0
        if batched:
            solver.iterate()
        else:
            assert sum(1 for _ in solver.create_iterator()) == 12
        rx, ry, _ = solver.timestepper.device.bedload_read()
        qbx, qby = model.get_bedload_term()
        assert np.array_equal(qbx, rx) and np.array_equal(qby, ry) and qbx.max() > 0
        res.append(_fields(solver) + [qbx.copy(), qby.copy()])
        assert solver.iteration == 12 and np.abs(res[-1][2] - bed0).max() > 0 and all(np.isfinite(a).all() for a in res[-1])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_trench_example(capsys):
    mod = _example()
    solver = mod.main(MESH + ['--steps', '24'])
    out = capsys.readouterr().out
    assert 'bedload transport' in out and 'bed change' in out and 'sediment_2d mass' in out
    assert solver.iteration == 24 and np.abs(solver.bed_change).max() > 0


def test_the_hump_moves_downstream(capsys):
    """bedload alone: the upstream face of the hump deepens, the lee face shoals, the centroid of the rise moves downstream"""
    mod = _example()
    solver = mod.main(['--bedload-only'] + MESH + ['--steps', '60', '--morfac', '500'])
    assert 'hump centroid' in capsys.readouterr().out
    x = solver.mesh2d.vertex_xy[:, 0]
    change = solver.bed_change
    up, lee = (x > 4.5) & (x < 5.7), (x > 6.3) & (x < 7.5)
    with capsys.disabled():
        print('hump: centroid {:.5f} -> {:.5f}, bed change {:+.3e} ... {:+.3e}'.format(*solver.centroids, change.min(), change.max()))
    assert (change[up] > 0).all() and (change[lee] < 0).all()
    assert solver.centroids[1] > solver.centroids[0] + 1e-4
    assert solver.iteration == 60 and (mod.HUMP_DEPTH - solver.fields.bathymetry_2d.dat.data_ro).max() > 0.5*mod.HUMP
