"""Particle sets on the device (csrc/swe2d_particles.hip): the kernel against the independent replay of tests/particle_cases.py bit
for bit - on the structured and the unstructured mesh, with wetting-drying, behind the buffer-swapping three-stage kernel, with long
moves, at the hop cap and at the edge sizes -; FlowSolver2d's batches with the callback against the step-by-step loop; the lifecycle
of the sets.
"""
import ctypes

import numpy as np
import pytest

from particle_cases import ACTIVE, EXITED, LOST, N_PARTICLES, Replay, random_particles, same_particles, scenario
from stats_cases import stats_mesh
from thetis_amd import DetectorsCallback, ParticleTrackerCallback, _lib
from thetis_amd.device import Swe2dDevice
from thetis_amd.mesh import RectangleMesh
from tide_cases import make_forcing, make_solver

pytestmark = pytest.mark.gpu


def _device(name, wd=False, fused3=False):
    mesh, bath, uv, eta, dt, dt_move, open_markers = scenario(name)
    dev = Swe2dDevice(mesh, bath, dt, boundary_len=mesh.boundary_len)
    assert dev.perm is not None and not np.array_equal(dev.perm, np.arange(mesh.num_cells))      # the cells read back are permuted
    if fused3:
        dev.set_option(_lib.OPT_FLOW, 0)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3)
    if wd:
        dev.set_wetting_and_drying(0.5)
    if name == 'coast':
        dev.set_bc(100, {'elev': 0.3})
        dev.set_bc(300, {'un': 0.0})
    dev.set_state(uv, eta)
    if fused3:
        on, tiles, ring1, ring2 = dev.fused_triple_info()
        assert on and tiles > 0 and ring1 > 0 and ring2 > 0, (on, tiles, ring1, ring2)
    return mesh, dev, dt_move, open_markers


def _move_and_replay(mesh, dev, dt_move, open_markers, n=N_PARTICLES, n_moves=10, seed=3):
    """n_moves times: one step, one move on the device, the same move in the replay from ``get_state``, and the comparison"""
    xy, cells = random_particles(mesh, n, seed=seed)
    pid = dev.particles_create(xy, cells)
    rp = Replay(mesh, xy, cells)
    first = dev.particles_read(pid)
    same_particles(first, rp.read(), 'as created')
    for j in range(n_moves):
        dev.advance(1)
        dev.particles_advance(pid, dt_move, open_markers)
        uv, eta = dev.get_state()
        assert np.isfinite(eta).all()
        rp.advance(uv, dt_move, open_markers)
        same_particles(dev.particles_read(pid), rp.read(), 'move {:d}'.format(j))
    assert not np.array_equal(rp.xy, xy) and (n < 256 or not np.array_equal(rp.cells, cells))
    dev.particles_destroy(pid)
    return rp


@pytest.mark.parametrize('name,wd,fused3', [('channel', False, False), ('coast', False, False), ('channel', True, False),
                                            ('channel', False, True)])
def test_device_equals_the_replay(hip_lib, name, wd, fused3):
    """700 particles (three workgroups, the last partial), 10 steps with a move after each: positions, cells, status, exit markers
    and wall hits equal the replay's after every move; no particle is lost (tests/test_particles.py checks that for the replay alone)"""
    mesh, dev, dt_move, open_markers = _device(name, wd=wd, fused3=fused3)
    rp = _move_and_replay(mesh, dev, dt_move, open_markers)
    print(name, wd, fused3, 'most cells', rp.most_cells, 'exited', int((rp.status == EXITED).sum()), 'wall hits', int(rp.hits.sum()))
    assert not (rp.status == LOST).any()
    assert rp.most_cells >= 2 and rp.hits.sum() > 0 and (rp.status == EXITED).any() and (rp.status == ACTIVE).any()
    assert set(rp.markers[rp.status == EXITED].tolist()) == set(open_markers)
    dev.close()


def test_long_moves(hip_lib):
    """moves across five and more cells, most of them ending at a wall or leaving"""
    mesh, dev, dt_move, open_markers = _device('long')
    rp = _move_and_replay(mesh, dev, dt_move, open_markers, n_moves=6)
    print('long: most cells', rp.most_cells, 'exited', int((rp.status == EXITED).sum()), 'wall hits', int(rp.hits.sum()))
    assert rp.most_cells >= 6 and rp.hits.sum() > 0 and (rp.status == EXITED).any() and not (rp.status == LOST).any()
    dev.close()


def test_hop_cap(hip_lib):
    """a move longer than the channel, 80 cells: the walks that would visit more than 64 cells end LOST, at their old positions, on
    the device and in the replay alike (a deterministic input of the cap, nothing faults)"""
    mesh, dev, dt_move, open_markers = _device('cap')
    xy, cells = random_particles(mesh, N_PARTICLES, seed=3)
    rp = _move_and_replay(mesh, dev, dt_move, open_markers, n_moves=1)
    lost = rp.status == LOST
    print('cap: lost', int(lost.sum()), 'most cells', rp.most_cells)
    assert lost.any() and rp.most_cells == 64 and (rp.status == EXITED).any()
    assert np.array_equal(rp.xy[lost], xy[lost]) and np.array_equal(rp.cells[lost], cells[lost])
    dev.close()


@pytest.mark.parametrize('n', [1, 256])
def test_edge_sizes(hip_lib, n):
    mesh, dev, dt_move, open_markers = _device('channel')
    _move_and_replay(mesh, dev, dt_move, open_markers, n=n, n_moves=3, seed=8)
    dev.close()


# ---- FlowSolver2d: batches
N_STEPS, EVERY, RECORD_EVERY, DT = 24, 4, 2, 0.3


def _solver_run(mode, with_particles=True, with_detectors=False):
    """24 steps on the 520 triangles with a tide on the device at marker 1; mode 'iterate' | 'loop'"""
    mesh = stats_mesh('triangles')
    forcing = make_forcing(mesh, K=3)
    s = make_solver(mesh, forcing, dt=DT, n_steps=N_STEPS, n_export=12)
    cb = det = None
    xy, _ = random_particles(mesh, 300, seed=12)
    if with_particles:
        cb = ParticleTrackerCallback(s, xy, every=EVERY, record_every=RECORD_EVERY, open_boundaries=(1,), export_to_hdf5=False,
                                     row_capacity=2)
        s.add_callback(cb, eval_interval='timestep')
    if with_detectors:
        det = DetectorsCallback(s, [(900.0, 700.0), (5100.0, 3300.0)], ['elev_2d', 'uv_2d'], 'gauges', export_to_hdf5=False)
        s.add_callback(det, eval_interval='timestep')
    dev = s.timestepper.device
    calls, moves = [], []
    inner, inner_move = dev.advance, dev.particles_advance
    dev.advance = lambda n=1: (calls.append(int(n)), inner(n))[1]
    dev.particles_advance = lambda pid, dt_move, open_markers=(): (moves.append(float(dt_move)), inner_move(pid, dt_move, open_markers))[1]
    if mode == 'iterate':
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == N_STEPS
    out = {'calls': calls, 'moves': moves, 'uv': s.fields.uv_2d.dat.data_ro.copy(), 'elev': s.fields.elev_2d.dat.data_ro.copy()}
    if cb is not None:
        out['state'] = (cb.positions(), cb.cells(), cb.status(), cb.exit_markers(), cb.wall_hits())
        out['traj'] = cb.trajectories()
        out['start'] = xy
    if det is not None:
        out['hist'] = (np.array([h[0] for h in det.history]), np.array([h[1] for h in det.history]))
    dev.close()
    return out


@pytest.fixture(scope='module')
def batched(hip_lib):
    return _solver_run('iterate')


def test_batched_equals_step_by_step(hip_lib, batched):
    loop = _solver_run('loop')
    assert loop['calls'] == [1]*N_STEPS and batched['calls'] == [EVERY]*(N_STEPS//EVERY)      # 6 advance calls
    assert batched['moves'] == loop['moves'] == [EVERY*DT]*(N_STEPS//EVERY)
    same_particles(batched['state'], loop['state'], 'iterate() against the loop')
    assert not np.array_equal(batched['state'][0], batched['start'])
    (t_b, rows_b), (t_l, rows_l) = batched['traj'], loop['traj']
    assert rows_b.shape == (N_STEPS//EVERY//RECORD_EVERY, 300, 2)                             # (through a row buffer of 2: drained once)
    assert np.array_equal(t_b, t_l) and np.array_equal(rows_b, rows_l) and np.array_equal(rows_b[-1], batched['state'][0])
    assert np.allclose(t_b, [8*DT, 16*DT, 24*DT], rtol=1e-15)
    plain = _solver_run('iterate', with_particles=False)
    assert plain['calls'] == [12, 12]
    for r in (batched, loop):
        assert np.array_equal(r['uv'], plain['uv']) and np.array_equal(r['elev'], plain['elev'])
    assert np.abs(plain['elev']).max() > 0.0


def test_detectors_next_to_the_tracker(hip_lib, batched):
    both = _solver_run('iterate', with_detectors=True)
    alone = _solver_run('iterate', with_particles=False, with_detectors=True)
    assert both['calls'] == alone['calls'] == [1]*N_STEPS                                     # a row per step: a call per step
    assert both['hist'][0].shape == (N_STEPS,)
    assert np.array_equal(both['hist'][0], alone['hist'][0]) and np.array_equal(both['hist'][1], alone['hist'][1])
    same_particles(both['state'], batched['state'], 'with detectors')
    assert np.array_equal(both['elev'], batched['elev'])


# ---- lifecycle
def _small_device():
    mesh, dev, _, _ = _device('channel')
    return mesh, dev


def _code(call):
    with pytest.raises(_lib.Swe2dError) as err:
        call()
    return err.value.code


def test_lifecycle(hip_lib):
    mesh, dev = _small_device()
    xy, cells = random_particles(mesh, 5, seed=2)
    a, b = dev.particles_create(xy, cells, capacity=2), dev.particles_create(xy[:3], cells[:3])
    assert (a, b) == (0, 1)
    assert dev.particles_read_rows(a).shape == (0, 5, 2)
    dev.particles_record(a)
    dev.advance(1)
    dev.particles_advance(a, 1200.0, (2,))
    dev.particles_record(a)
    moved = dev.particles_read(a)[0]
    assert _code(lambda: dev.particles_record(a)) == _lib.ERR_INVALID_ARGUMENT              # full: refused, nothing written
    assert _code(lambda: dev.particles_record(b)) == _lib.ERR_INVALID_ARGUMENT              # capacity 0
    rows = dev.particles_read_rows(a)
    assert rows.shape == (2, 5, 2) and np.array_equal(rows[0], xy) and np.array_equal(rows[1], moved) and not np.array_equal(moved, xy)
    assert dev.particles_read_rows(a).shape == (0, 5, 2)                                    # read_rows empties the buffer
    dev.particles_record(a)
    assert np.array_equal(dev.particles_read_rows(a)[0], moved)
    untouched = dev.particles_read(b)                                                       # two sets do not disturb each other
    assert np.array_equal(untouched[0], xy[:3]) and np.array_equal(untouched[1], cells[:3]) and (untouched[2] == ACTIVE).all()
    dev.particles_destroy(a)                                                                # a destroyed id is refused ...
    for call in (lambda: dev.particles_advance(a, 1.0), lambda: dev.particles_record(a), lambda: dev.particles_read(a),
                 lambda: dev.particles_read_rows(a), lambda: dev.particles_destroy(a)):
        assert _code(call) == _lib.ERR_INVALID_ARGUMENT
    assert dev.particles_create(xy, cells, capacity=1) == a                                 # ... and reused
    # create: a cell out of range, a position outside its cell, bad sizes; the handle stays usable after each
    assert _code(lambda: dev.particles_create(xy, np.full(5, mesh.num_cells))) == _lib.ERR_INVALID_ARGUMENT
    bad = np.ascontiguousarray(np.full(5, mesh.num_cells, dtype=np.int32))
    pid = ctypes.c_int32()
    rc = dev.lib.swe2d_particles_create(dev.h, 5, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0, ctypes.byref(pid))
    assert rc == _lib.ERR_INVALID_ARGUMENT                                                  # (the C entry point itself)
    assert _code(lambda: dev.particles_create(xy, np.roll(cells, 1))) == _lib.ERR_INVALID_ARGUMENT
    assert _code(lambda: dev.particles_create(xy, cells, capacity=-1)) == _lib.ERR_INVALID_ARGUMENT
    assert _code(lambda: dev.particles_advance(a, float('nan'))) == _lib.ERR_INVALID_ARGUMENT
    dev.advance(1)
    dev.particles_advance(a, 1200.0)
    assert np.isfinite(dev.particles_read(a)[0]).all() and np.isfinite(dev.get_state()[1]).all()
    assert dev.particles_create(xy, cells) == 2
    dev.close()                                                                             # swe2d_destroy with three live sets


def test_quadrilaterals_are_unsupported(hip_lib):
    mesh = RectangleMesh(6, 4, 6000.0, 4000.0, quadrilateral=True)
    dev = Swe2dDevice(mesh, np.full(mesh.num_vertices, 10.0), 0.5)
    dev.set_state(np.zeros((mesh.num_cells, 4, 2)), np.zeros((mesh.num_cells, 4)))
    assert _code(lambda: dev.particles_create([(100.0, 100.0)], [0])) == _lib.ERR_UNSUPPORTED
    dev.advance(1)                                                                          # the handle is usable
    assert np.isfinite(dev.get_state()[1]).all()
    dev.close()


def test_refused_inside_a_stream_capture(hip_lib):
    import torch
    mesh, dev = _small_device()
    xy, cells = random_particles(mesh, 9, seed=4)
    pid = dev.particles_create(xy, cells, capacity=1)
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        buf = torch.zeros(16, device='cuda')
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            buf.add_(1.0)                                     # (the capture records something; nothing is replayed)
            for call in (lambda: dev.particles_advance(pid, 1200.0), lambda: dev.particles_create(xy, cells),
                         lambda: dev.particles_record(pid), lambda: dev.particles_read(pid), lambda: dev.particles_read_rows(pid),
                         lambda: dev.particles_destroy(pid)):
                assert _code(call) == _lib.ERR_UNSUPPORTED
        s.synchronize()
        dev.advance(1)                                        # the handle is usable, the set untouched
        dev.particles_advance(pid, 1200.0, (2,))
        got = dev.particles_read(pid)
    dev.set_stream(None)
    rp = Replay(mesh, xy, cells)
    rp.advance(dev.get_state()[0], 1200.0, (2,))
    same_particles(got, rp.read(), 'after the capture')
    dev.close()
