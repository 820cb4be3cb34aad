"""Particle tracking on the host (thetis_amd/particles.py): known answers of the midpoint walk in uniform flow and in solid-body
rotation, the numpy implementation against the independent replay of tests/particle_cases.py, the sampling schedule through
FlowSolver2d on the host stand-in device, the file, the refusals, and the ABI of the built library."""
import ctypes
import math
import os
import types

import numpy as np
import pytest

from cpu_device import CpuSwe2dDevice
from particle_cases import ACTIVE, EXITED, LOST, N_PARTICLES, Replay, random_particles, rotated, same_particles, scenario
from thetis_amd import Constant, ParticleTrackerCallback, PointNotInDomainError, _lib, callback, particles, solver2d
from thetis_amd.mesh import RectangleMesh
from tide_cases import make_solver
from stats_cases import stats_mesh

EPS = float(np.finfo(np.float64).eps)


def _bare(mesh, uv, dt, positions, **kw):
    """a callback on a solver stand-in without a device: ``step()`` counts one time step and evaluates the callback in ``uv``"""
    holder = {'uv': np.asarray(uv, dtype=np.float64)}
    solver = types.SimpleNamespace(comm=types.SimpleNamespace(size=1, rank=0), simulation_time=0.0, iteration=0, dt=dt, mesh2d=mesh,
                                   fields=types.SimpleNamespace(uv_2d=types.SimpleNamespace(cell_node_values=lambda: holder['uv'])),
                                   timestepper=types.SimpleNamespace())
    cb = ParticleTrackerCallback(solver, positions, export_to_hdf5=False, **kw)

    def step(n=1):
        for _ in range(n):
            solver.iteration += 1
            solver.simulation_time = solver.iteration*dt
            cb.evaluate()
    return cb, step, holder


def test_exported_from_the_package_and_from_callback():
    assert callback.ParticleTrackerCallback is particles.ParticleTrackerCallback is ParticleTrackerCallback
    assert 'ParticleTrackerCallback' in callback.__all__
    assert (ACTIVE, EXITED, LOST) == (particles.ACTIVE, particles.EXITED, particles.LOST) == (0, 1, 2)


# ---- uniform flow (U, 0) on 1000 m x 400 m, markers 1: x = 0, 2: x = 1000, 3 / 4: the sides
LX, LY, U, DT = 1000.0, 400.0, 0.5, 10.0


def _uniform():
    mesh = RectangleMesh(10, 4, LX, LY)
    uv = np.zeros((mesh.num_cells, 3, 2))
    uv[:, :, 0] = U
    return mesh, uv


@pytest.mark.parametrize('every', [1, 3])
def test_uniform_flow_displaces_by_every_dt_u(every):
    """x' = x + dt_move*(l0*U + l1*U + l2*U): the weights sum to 1 within 2 eps, the product and the sum round once each: the
    displacement is every*dt*U within 4 eps of the coordinate's scale (1000 m), through every cell the path crosses"""
    mesh, uv = _uniform()
    start = np.array([[12.5, 40.0], [333.3, 199.9], [99.999, 371.0]])
    cb, step, _ = _bare(mesh, uv, DT, start, every=every)
    for j in range(1, 7):
        before = cb.positions()
        step(every)
        after = cb.positions()
        assert np.abs(after[:, 0] - before[:, 0] - every*DT*U).max() <= 4*EPS*LX
        assert np.array_equal(after[:, 1], before[:, 1])
    assert cb.n_advances == 6 and (cb.status() == ACTIVE).all() and (cb.wall_hits() == 0).all()
    xy = mesh.cell_xy()[cb.cells()]
    assert ((after[:, 0] >= xy[:, :, 0].min(axis=1)) & (after[:, 0] <= xy[:, :, 0].max(axis=1))).all()      # the cells followed


def test_uniform_flow_leaves_through_an_open_boundary_on_time():
    d = 22.0
    n_exit = math.ceil(d/(U*DT))
    assert n_exit == 5
    mesh, uv = _uniform()
    cb, step, _ = _bare(mesh, uv, DT, [(LX - d, 130.0), (400.0, 130.0)], open_boundaries=(2,))
    step(n_exit - 1)
    assert cb.status().tolist() == [ACTIVE, ACTIVE] and cb.exit_markers().tolist() == [0, 0]
    step(1)
    assert cb.status().tolist() == [EXITED, ACTIVE] and cb.exit_markers().tolist() == [2, 0]
    frozen = cb.positions()[0]
    assert abs(frozen[0] - LX) <= 4*EPS*LX and frozen[1] == 130.0
    step(3)                                                   # an EXITED particle is never touched again
    assert np.array_equal(cb.positions()[0], frozen) and cb.status()[0] == EXITED
    assert abs(cb.positions()[1, 0] - (400.0 + 8*DT*U)) <= 32*EPS*LX


def test_uniform_flow_stops_at_a_wall():
    d = 22.0
    mesh, uv = _uniform()
    cb, step, _ = _bare(mesh, uv, DT, [(LX - d, 130.0)])      # marker 2 not listed: a wall
    step(8)
    x, y = cb.positions()[0]
    assert cb.status()[0] == ACTIVE and cb.wall_hits()[0] > 0 and cb.exit_markers()[0] == 0
    assert LX - 2.0**-10*(U*DT) <= x <= LX and y == 130.0
    lam = particles.HostParticles._facet_coordinates(cb._host._geometry(cb.cells().astype(np.int64)), np.array([x]), np.array([y]))
    assert min(float(m[0]) for m in lam) >= 0.0               # inside its cell, hence inside the mesh


# ---- solid-body rotation
ROTATION_MEASURED = 3.1e-12     # m: the worst |host path - closed form| over the 200 steps, measured on the CPU (radii up to 150 m)


def test_solid_body_rotation_follows_the_closed_form():
    """u = (-w (y - yc), w (x - xc)) is in P1, so the tracker integrates it as the midpoint rule does: with th = w*dt a rotation by
    atan2(th, 1 - th^2/2) and a radial factor sqrt(1 + th^4/4) per step.  200 steps of th = 0.05 (1.6 turns, through about 100
    cells each) stay within 10 x the deviation measured for the host path, 3.1e-12 m (ROTATION_MEASURED: round-off of 200 steps at
    coordinates of 1e3 m - 200 * 4 eps * 1e3 = 1.8e-10 would be the plain bound); an error of the algorithm shows at th^3 * r =
    2e-2 m per step."""
    mesh = RectangleMesh(10, 4, LX, LY)
    centre = np.array([0.5*LX, 0.5*LY])
    w, dt = 0.005, 10.0
    th = w*dt
    cxy = mesh.cell_xy()
    uv = np.stack([-w*(cxy[:, :, 1] - centre[1]), w*(cxy[:, :, 0] - centre[0])], axis=2)
    start = centre + np.array([[150.0, 0.0], [0.0, -120.0], [-33.0, 71.0], [5.0, 2.5], [-100.0, -100.0]])
    cb, step, _ = _bare(mesh, uv, dt, start)
    worst = 0.0
    for j in range(1, 201):
        step()
        worst = max(worst, float(np.abs(cb.positions() - rotated(start, centre, j, th)).max()))
    print('rotation: worst |host - closed form| = {:.3e} m over 200 steps'.format(worst))
    assert (cb.status() == ACTIVE).all() and (cb.wall_hits() == 0).all()
    assert len(set(cb.cells().tolist())) > 1
    assert worst <= 10*ROTATION_MEASURED, worst


# ---- the numpy implementation against the independent replay
@pytest.mark.parametrize('case', ['channel', 'coast', 'long', 'cap'])
def test_host_particles_equal_the_replay(case):
    """the scenarios of tests/test_gpu_particles.py with the state frozen - random velocities strong enough for cell crossings, walls
    and exits ('long': five and more cells per move; 'cap': moves that reach the 64-cell cap): positions, cells, status, exit markers
    and wall hits of HostParticles equal the replay's after every move, bit for bit, and but for 'cap' the replay loses no particle"""
    mesh, _, uv, _, _, dt, open_markers = scenario(case)
    xy, _ = random_particles(mesh, N_PARTICLES, seed=3)
    cb, step, _ = _bare(mesh, uv, dt, xy, open_boundaries=open_markers)
    rp = Replay(mesh, xy, cb.initial_cells)
    for j in range(10):
        step()
        rp.advance(uv, dt, open_markers)
        same_particles((cb.positions(), cb.cells(), cb.status(), cb.exit_markers(), cb.wall_hits()), rp.read(), '{:} move {:d}'.format(case, j))
    st = rp.status
    print(case, 'most cells in a walk', rp.most_cells, 'exited', int((st == EXITED).sum()), 'lost', int((st == LOST).sum()),
          'wall hits', int(rp.hits.sum()))
    if case == 'cap':
        assert (st == LOST).any() and rp.most_cells == 64
    else:
        assert not (st == LOST).any() and rp.hits.sum() > 0 and (st == EXITED).any()
    if case == 'long':
        assert rp.most_cells >= 6
    if case in ('channel', 'coast'):
        assert rp.most_cells >= 2


# ---- through FlowSolver2d on the host stand-in
def _host_solver(n_steps, n_export, outdir=None):
    return make_solver(stats_mesh('triangles'), Constant(0.2), dt=0.3, n_steps=n_steps, n_export=n_export, outdir=outdir)


@pytest.mark.parametrize('batch', [True, False])
def test_callback_equals_the_replay_and_keeps_its_schedule(ref_so, monkeypatch, batch):
    """every = 3 inside the window [5 dt -, 17 dt +], record_every = 2: of 20 steps the iterations 6, 9, 12, 15 move the particles
    by 3 dt, 9 and 15 leave a row.  The replay, driven by hand from ``get_state`` of a second run without the callback, gives the
    same positions, cells and status bit for bit; the device class has no particle sets, so iterate() goes step by step."""
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    dt = 0.3
    s = _host_solver(20, 10)
    xy, _ = random_particles(s.mesh2d, 40, seed=5)
    cb = ParticleTrackerCallback(s, xy, every=3, record_every=2, open_boundaries=(1,), start_time=4.9*dt, end_time=17.1*dt,
                                 export_to_hdf5=False)
    s.add_callback(cb, eval_interval='timestep')
    if batch:
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == 20
    twin = _host_solver(20, 10)
    rp = Replay(twin.mesh2d, xy, cb.initial_cells)
    moved, rows, times = [], [], []
    for _ in twin.create_iterator():
        it = twin.iteration + 1                                # (the generator yields before the counters move on)
        if it % 3 == 0 and 4.9*dt <= it*dt <= 17.1*dt:
            rp.advance(twin.timestepper.device.get_state()[0], 3*dt, (1,))
            moved.append(it)
            if len(moved) % 2 == 0:
                rows.append(rp.xy.copy())
                times.append(it*dt)
    assert moved == [6, 9, 12, 15] and cb.n_advances == 4
    same_particles((cb.positions(), cb.cells(), cb.status(), cb.exit_markers(), cb.wall_hits()), rp.read(), 'solver')
    assert not np.array_equal(cb.positions(), xy)
    t, traj = cb.trajectories()
    assert traj.shape == (2, 40, 2) and np.array_equal(t, np.array(times)) and np.array_equal(traj, np.array(rows))
    assert np.array_equal(cb.trajectories()[1], traj)           # reading twice gives the same rows
    assert np.array_equal(s.fields.elev_2d.dat.data_ro, twin.fields.elev_2d.dat.data_ro)


def test_export_writes_the_npz(ref_so, monkeypatch, tmp_path):
    monkeypatch.setattr(solver2d.FlowSolver2d, '_device_cls', CpuSwe2dDevice, raising=False)
    s = _host_solver(6, 3)
    xy, _ = random_particles(s.mesh2d, 7, seed=1)
    cb = ParticleTrackerCallback(s, xy, name='drifters', record_every=2, outputdir=str(tmp_path))
    s.add_callback(cb, eval_interval='timestep')
    s.iterate()
    d = np.load(os.path.join(str(tmp_path), 'diagnostic_drifters.npz'))
    assert d['trajectories'].shape == (3, 7, 2) and np.allclose(d['time'], [0.6, 1.2, 1.8], rtol=1e-15)
    assert np.array_equal(d['positions'], cb.positions()) and np.array_equal(d['trajectories'][-1], d['positions'])
    assert np.array_equal(d['initial_positions'], xy) and int(d['n_advances']) == 6
    for key, dtype in (('cells', np.int32), ('status', np.int32), ('exit_markers', np.int32), ('wall_hits', np.int32)):
        assert d[key].shape == (7,) and d[key].dtype == dtype
    assert np.array_equal(cb.excursion(), np.hypot(*(d['positions'] - xy).T))


# ---- refusals
def test_a_point_outside_the_mesh_is_refused():
    mesh, uv = _uniform()
    with pytest.raises(PointNotInDomainError):
        _bare(mesh, uv, DT, [(10.0, 10.0), (LX + 1.0, 10.0)])


def test_quadrilaterals_are_refused_at_construction():
    mesh = RectangleMesh(4, 3, LX, LY, quadrilateral=True)
    with pytest.raises(NotImplementedError, match='triangles'):
        _bare(mesh, np.zeros((mesh.num_cells, 4, 2)), DT, [(10.0, 10.0)])


def test_several_ranks_are_refused_at_the_first_evaluation():
    mesh, uv = _uniform()
    cb, step, _ = _bare(mesh, uv, DT, [(10.0, 10.0)])
    cb.solver_obj.comm.size = 2
    with pytest.raises(NotImplementedError, match='several ranks'):
        step()


def test_bad_intervals_are_refused():
    mesh, uv = _uniform()
    for kw in ({'every': 0}, {'record_every': 0}):
        with pytest.raises(ValueError):
            _bare(mesh, uv, DT, [(10.0, 10.0)], **kw)


def test_abi_of_the_built_library():
    """if the library is built: the six swe2d_particles_* symbols resolve and the ABI version is still 12"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libswe2d_hip.so is not built')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('swe2d_particles_create', 'swe2d_particles_advance', 'swe2d_particles_record', 'swe2d_particles_read',
                 'swe2d_particles_read_rows', 'swe2d_particles_destroy'):
        assert getattr(lib, name) is not None and name in _lib.SYMBOLS
    assert lib.swe2d_abi_version() == 12 == _lib.ABI_VERSION
