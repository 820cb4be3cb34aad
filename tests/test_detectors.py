"""CPU tests of point location (thetis_amd/pointeval.py), Function.at on host functions and the detector callbacks
(thetis_amd/callback.py) driven through the host stand-in device; partitioned runs under gloo give the single-rank series."""
import os

import numpy as np
import pytest

from helpers import delaunay_case, quad_case
from thetis_amd import DetectorsCallback, Function, PointNotInDomainError, TimeSeriesCallback2D, get_functionspace, \
    select_and_move_detectors
from thetis_amd.mesh import PeriodicRectangleMesh, RectangleMesh
from thetis_amd.pointeval import PointLocator, evaluate


def _affine_check(mesh, pts):
    loc = PointLocator(mesh, pts)
    assert (loc.cells >= 0).all()
    P = mesh.cell_xy()
    f = 3.0 + 2e-3*P[..., 0] - 5e-3*P[..., 1]
    exact = 3.0 + 2e-3*pts[:, 0] - 5e-3*pts[:, 1]
    assert np.abs(evaluate(f, loc.cells, loc.weights) - exact).max() <= 1e-12*np.abs(exact).max()
    assert np.allclose(loc.weights.sum(axis=1), 1.0, rtol=0, atol=1e-13)


def _interior(rng, lx, ly, n=400, skew=0.0):
    pts = rng.uniform([1e-3*lx, 1e-3*ly], [(1 - 1e-3)*lx, (1 - 1e-3)*ly], size=(n, 2))
    pts[:, 0] += skew*pts[:, 1]
    return pts


@pytest.mark.parametrize('diagonal', ['left', 'right'])
def test_locator_rectangle_mesh(diagonal):
    _affine_check(RectangleMesh(17, 9, 1e4, 5e3, diagonal=diagonal), _interior(np.random.default_rng(1), 1e4, 5e3))


def test_locator_delaunay_mesh():
    mesh = delaunay_case()[0]
    _affine_check(mesh, _interior(np.random.default_rng(2), 10e3, 6e3))


def test_locator_parallelogram_quadrilaterals():
    mesh = quad_case(skew=0.3)[0]
    _affine_check(mesh, _interior(np.random.default_rng(3), 100e3, 30e3, skew=0.3))


def test_locator_general_quadrilaterals():
    mesh = quad_case(warp=0.3)[0]
    assert not mesh.affine
    _affine_check(mesh, _interior(np.random.default_rng(4), 100e3, 30e3))


def test_locator_periodic_mesh():
    _affine_check(PeriodicRectangleMesh(10, 6, 1e4, 6e3), _interior(np.random.default_rng(5), 1e4, 6e3))


def test_locator_large_mesh_has_no_cells_times_points_loop():
    """10 000 points on 2 M triangles: buckets, not a scan of every cell per point"""
    import time
    mesh = RectangleMesh(1000, 1000, 1.0, 1.0)
    pts = np.random.default_rng(6).uniform(0, 1, size=(10000, 2))
    t0 = time.perf_counter()
    loc = PointLocator(mesh, pts)
    assert (loc.cells >= 0).all()
    assert time.perf_counter() - t0 < 30.0


def test_tie_rule_picks_the_lowest_cell():
    for mesh in (RectangleMesh(6, 4, 6.0, 4.0), RectangleMesh(6, 4, 6.0, 4.0, quadrilateral=True), delaunay_case(60)[0]):
        P = mesh.cell_xy()
        k = P.shape[1]
        verts = mesh.vertex_xy
        mids = 0.5*(P + np.roll(P, -1, axis=1)).reshape(-1, 2)
        pts = np.concatenate([verts, mids])
        loc = PointLocator(mesh, pts)
        assert (loc.cells >= 0).all()
        for p, c in zip(pts, loc.cells):
            # every cell whose closure holds the point: the lowest one wins
            holders = []
            for cell in range(mesh.num_cells):
                ok, _ = PointLocator._reference_coordinates(P[cell:cell + 1], p[None], 1e-10)
                if ok[0]:
                    holders.append(cell)
            assert c == min(holders)
        assert k in (3, 4)


def test_outside_points():
    mesh = RectangleMesh(4, 3, 4.0, 3.0)
    f = Function(get_functionspace(mesh, 'CG', 1)).interpolate(lambda x, y: 1.0 + x + 2*y)
    with pytest.raises(PointNotInDomainError):
        f.at((5.0, 1.0))
    assert f.at((5.0, 1.0), dont_raise=True) is None
    out = f.at([(1.0, 1.0), (5.0, 1.0)], dont_raise=True)
    assert out[1] is None and abs(out[0] - 4.0) < 1e-14
    assert abs(f.at((0.5, 0.25)) - 2.0) < 1e-14
    assert np.allclose(f.at((0.5, 0.25), (1.0, 1.0)), [2.0, 4.0], rtol=0, atol=1e-14)
    v = Function(get_functionspace(mesh, 'DG', 1, vector=True)).interpolate(lambda x, y: (x, -y))
    assert v.at((1.5, 2.5)).shape == (2,) and np.allclose(v.at((1.5, 2.5)), [1.5, -2.5], rtol=0, atol=1e-14)


def test_select_and_move_detectors():
    """test/swe2d/test_standing_wave.py of the reference"""
    lx, ly, nx = 5e3, 1e3, 100
    mesh = RectangleMesh(nx, 1, lx, ly)
    xy = [[-2*lx, ly/2.], [-lx/2, ly/2.], [lx/4., ly/2.], [3*lx/4., ly/2.]]
    moved = select_and_move_detectors(mesh, xy, maximum_distance=lx)
    assert len(moved) == 3
    np.testing.assert_almost_equal(moved[0][0], lx/nx/3.)
    moved, names = select_and_move_detectors(mesh, xy, detector_names=['a', 'b', 'c', 'd'], maximum_distance=lx)
    assert names == ['b', 'c', 'd']
    assert len(select_and_move_detectors(mesh, xy)) == 2


def _stand_in_solver(tmp_path, monkeypatch):
    from detector_cases import CpuProbeDevice
    from thetis_amd import solver2d
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuProbeDevice, raising=False)
    mesh = RectangleMesh(10, 2, 10e3, 2e3)
    bath = Function(get_functionspace(mesh, 'CG', 1)).assign(10.0)
    s = solver2d.FlowSolver2d(mesh, bath)
    s.options.timestep = 10.0
    s.options.simulation_export_time = 30.0
    s.options.simulation_end_time = 60.0
    s.options.no_exports = True
    s.options.output_directory = str(tmp_path)
    s.options.swe_timestepper_type = 'SSPRK33'
    s.options.swe_timestepper_options.use_automatic_timestep = False
    s.create_equations()
    s.assign_initial_conditions(elev=Function(get_functionspace(mesh, 'CG', 1)).interpolate(lambda x, y: 0.1*np.cos(np.pi*x/10e3)))
    return s


def test_callback_surface(tmp_path, monkeypatch, capsys):
    s = _stand_in_solver(tmp_path, monkeypatch)
    xy = [(1e3, 1e3), (5e3, 5e2), (9e3, 1.5e3)]
    cb = DetectorsCallback(s, xy, ['elev_2d', 'uv_2d'], 'set1', append_to_log=True)
    assert cb.name == 'set1' and cb.detector_names == ['detector0', 'detector1', 'detector2'] and cb.field_dims == [1, 2]
    assert cb.variable_names == cb.detector_names
    cb2 = DetectorsCallback(s, xy, ['elev_2d'], 'set2', detector_names=['x', 'y', 'z'])
    assert cb2.append_to_log is False
    ts = TimeSeriesCallback2D(s, ['elev_2d', 'uv_2d'], 5e3, 5e2, 'mid')
    assert ts.name == 'timeseries_mid_elev_2d-uv_2d'
    s.add_callback(cb, 'export')
    s.add_callback(cb2, 'timestep')
    s.add_callback(ts, 'timestep')
    s.iterate()
    # history: (t, (detectors, sum of dims)) per evaluation
    assert [h[0] for h in cb.history] == [0.0, 30.0, 60.0]
    assert all(h[1].shape == (3, 3) for h in cb.history)
    assert [h[0] for h in cb2.history] == [10.0*k for k in range(1, 7)]
    out = capsys.readouterr().out
    assert 'In detector1: elev_2d=[' in out and ', uv_2d=[' in out
    msg = cb.message_str(*cb.history[-1][1])
    assert msg.splitlines()[0].startswith('In detector0: elev_2d=[')
    # the values are the host evaluation of the state
    uv = s.fields.uv_2d.cell_node_values()
    eta = s.fields.elev_2d.cell_node_values()
    loc = PointLocator(s.mesh2d, xy)
    assert np.array_equal(cb.history[-1][1][:, 0], evaluate(eta, loc.cells, loc.weights))
    assert np.array_equal(cb.history[-1][1][:, 1:], evaluate(uv, loc.cells, loc.weights))
    assert np.array_equal(s.fields.elev_2d.at(xy), cb.history[-1][1][:, 0])
    # the file
    with np.load(os.path.join(str(tmp_path), 'diagnostic_set1.npz')) as z:
        assert z['time'].shape == (3, 1) and z['detector2'].shape == (3, 3)
        assert list(z['field_names']) == ['elev_2d', 'uv_2d'] and list(z['field_dims']) == [1, 2]
        assert list(z['detector_names']) == cb.detector_names and z['detector_xy'].shape == (3, 2)
    with np.load(os.path.join(str(tmp_path), 'diagnostic_set2.npz')) as z:
        assert z['time'][:, 0].tolist() == [10.0*k for k in range(1, 7)] and z['y'].shape == (6, 1)


def test_no_file_without_export(tmp_path, monkeypatch):
    s = _stand_in_solver(tmp_path, monkeypatch)
    s.add_callback(DetectorsCallback(s, [(1e3, 1e3)], ['elev_2d'], 'quiet', export_to_hdf5=False), 'timestep')
    s.iterate()
    assert not os.path.exists(os.path.join(str(tmp_path), 'diagnostic_quiet.npz'))


def test_detector_outside_raises_with_its_name(tmp_path, monkeypatch):
    s = _stand_in_solver(tmp_path, monkeypatch)
    cb = DetectorsCallback(s, [(1e3, 1e3), (-5.0, 1e3)], ['elev_2d'], 'bad', detector_names=['in', 'out'])
    with pytest.raises(PointNotInDomainError, match='out'):
        cb()


def test_batched_rows_equal_the_step_loop(tmp_path, monkeypatch):
    """iterate() batches the steps between exports with a row after every step; create_iterator() steps one by one"""
    from detector_cases import channel_with_detectors, result, assert_same
    from detector_cases import CpuProbeDevice
    from thetis_amd import solver2d
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuProbeDevice, raising=False)
    calls = []
    orig = CpuProbeDevice.advance
    monkeypatch.setattr(CpuProbeDevice, 'advance', lambda self, n=1: (calls.append(n), orig(self, n))[1])
    a = result(channel_with_detectors(str(tmp_path / 'a')), str(tmp_path / 'a'))
    n_batched = len(calls)
    monkeypatch.setattr(solver2d.FlowSolver2d, 'iterate', lambda self, update_forcings=None, export_func=None:
                        [None for _ in self.create_iterator(update_forcings, export_func)])
    b = result(channel_with_detectors(str(tmp_path / 'b')), str(tmp_path / 'b'))
    assert_same(a, b)
    assert len(a['gauges'][0]) == 80 and a['gauges'][1].shape == (80, 21, 3)


@pytest.mark.parametrize('world', [2, 3])
def test_partitioned_detectors_equal_single_rank(tmp_path, ref_so, world):
    from detector_cases import run_detectors, assert_same
    single = run_detectors(1, str(tmp_path / 'one'))[0]
    for r in run_detectors(world, str(tmp_path / 'many')):
        assert_same(single, r)
