"""Random-walk dispersion, timed releases and cell counts of particle sets on the device (csrc/swe2d_particles.hip) against
``particles.HostParticles`` bit for bit: constant and varying diffusivity, second walks that end at walls, exits and the hop cap, the
edge sizes, independence of a particle's deviates from its company and from batching, the release gate, the counts, the lifecycle of
the new calls, and examples/particle_plume.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from particle_cases import ACTIVE, EXITED, LOST, random_particles, same_particles, scenario
from particle_walk_cases import walk_scenario
from stats_cases import stats_mesh
from thetis_amd import ParticleTrackerCallback, _lib
from thetis_amd.device import Swe2dDevice
from thetis_amd.mesh import RectangleMesh
from thetis_amd.particles import HostParticles
from tide_cases import make_forcing, make_solver

pytestmark = pytest.mark.gpu
WAITING = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(name):
    mesh, bath, uv, eta, dt, dt_move, open_markers = scenario(name)
    dev = Swe2dDevice(mesh, bath, dt, boundary_len=mesh.boundary_len)
    assert dev.perm is not None and dev._vperm is not None                   # cells and vertices are renumbered on the device
    if name == 'coast':
        dev.set_bc(100, {'elev': 0.3})
        dev.set_bc(300, {'un': 0.0})
    dev.set_state(uv, eta)
    return mesh, dev, dt_move, open_markers


def _host(mesh, xy, cells):
    return HostParticles(mesh.cells, mesh.vertex_xy, mesh.cell_nbr, mesh.cell_nbr_facet, xy, cells)


def _pair(mesh, dev, xy, cells, K=None, seed=0, release=None):
    """the same set on the device and on the host"""
    pid, host = dev.particles_create(xy, cells), _host(mesh, xy, cells)
    if K is not None:
        dev.particles_set_diffusivity(pid, K, seed)
        host.set_diffusivity(K, seed)
    if release is not None:
        dev.particles_set_release_times(pid, release, 0.0)
        host.set_release_times(release, 0.0)
    same_particles(dev.particles_read(pid), host.read(), 'as created')
    return pid, host


def _moves(dev, pairs, dt_move, open_markers, n_moves):
    """n_moves times: one step, one move of every (set, host) pair in the state it left, the comparison"""
    t = 0.0
    for j in range(n_moves):
        dev.advance(1)
        t += dt_move
        for pid, _ in pairs:
            dev.particles_advance_at(pid, dt_move, t, open_markers)
        uv, eta = dev.get_state()
        assert np.isfinite(eta).all()
        for pid, host in pairs:
            host.advance_at(uv, dt_move, t, open_markers)
            same_particles(dev.particles_read(pid), host.read(), 'move {:d}'.format(j))


@pytest.mark.parametrize('name', ['channel', 'coast'])
@pytest.mark.parametrize('kind', ['constant', 'varying', 'strong'])
def test_device_equals_the_host(hip_lib, name, kind):
    """700 particles, 10 steps with a move after each: positions, cells, status, exit markers and wall hits equal HostParticles'
    after every move.  'strong' walks up to three cells per move: its second walks end at walls and at open boundaries - a
    twin without diffusivity shows that these are not the midpoint move's."""
    mesh, dev, dt_move, open_markers = _device(name)
    xy, cells = random_particles(mesh, 700, seed=3)
    K, seed = walk_scenario(name, kind)
    walk, plain = _pair(mesh, dev, xy, cells, K, seed), _pair(mesh, dev, xy, cells)
    _moves(dev, [walk, plain], dt_move, open_markers, 10)
    h, p = walk[1], plain[1]
    print(name, kind, 'exited', int((h.status == EXITED).sum()), 'of them without the walk', int((p.status == EXITED).sum()),
          'wall hits', int(h.hits.sum()), int(p.hits.sum()))
    assert not np.array_equal(h.xy, p.xy) and not (h.status == LOST).any() and (h.status == ACTIVE).any()
    if kind == 'strong':
        assert h.hits.sum() > p.hits.sum() + 50 and (h.status == EXITED).sum() > (p.status == EXITED).sum() + 10
        assert h.hits.max() >= 2
    for status in ((ACTIVE,), (EXITED,), (ACTIVE, EXITED)):
        c = dev.particles_cell_counts(walk[0], status)
        assert c.dtype == np.int32 and np.array_equal(c, h.cell_counts(status)) and c.sum() == np.isin(h.status, status).sum()
    dev.close()


def test_lost_in_the_second_walk(hip_lib):
    """80 cells along the channel and random-walk steps of up to 120 km: walks that would visit more than 64 cells end LOST at the
    position before the whole advance, with nothing else written; the midpoint move (1.2 km) loses nobody"""
    mesh, dev, _, open_markers = _device('cap')
    xy, cells = random_particles(mesh, 700, seed=3)
    walk, plain = _pair(mesh, dev, xy, cells, 2.0e6, 5), _pair(mesh, dev, xy, cells)
    _moves(dev, [walk, plain], 1200.0, open_markers, 1)
    lost = walk[1].status == LOST
    print('lost', int(lost.sum()), 'exited', int((walk[1].status == EXITED).sum()))
    assert lost.any() and not (plain[1].status == LOST).any()
    assert np.array_equal(walk[1].xy[lost], xy[lost]) and (walk[1].hits[lost] == 0).all()
    dev.close()


@pytest.mark.parametrize('n', [1, 256, 257, 700])
def test_set_sizes(hip_lib, n):
    mesh, dev, dt_move, open_markers = _device('channel')
    xy, cells = random_particles(mesh, n, seed=8)
    K, seed = walk_scenario('channel', 'varying')
    release = 2.0*dt_move*np.arange(n)/n
    _moves(dev, [_pair(mesh, dev, xy, cells, K, seed), _pair(mesh, dev, xy, cells, K, seed, release)], dt_move, open_markers, 3)
    dev.close()


def test_a_particle_does_not_depend_on_its_company(hip_lib):
    """set b is set a in which the odd particles left first: the even ones wait while one very long plain move takes the odd ones
    through boundaries that are all open; then everybody is released.  The even particles of both sets then make the same ten
    moves: the counter of the deviates is (index, move), not a position in a compacted list"""
    mesh, dev, dt_move, open_markers = _device('channel')
    xy, cells = random_particles(mesh, 700, seed=3)
    K, seed = walk_scenario('channel', 'varying')
    odd = np.arange(700) % 2 == 1
    a = dev.particles_create(xy, cells)
    b = dev.particles_create(xy, cells)
    dev.particles_set_release_times(b, np.where(odd, -np.inf, np.inf), 0.0)
    dev.particles_advance(b, 1.0e8, (1, 2, 3, 4))                            # the old entry point: no move is counted
    dev.particles_set_release_times(b, np.full(700, -np.inf), 0.0)
    first = dev.particles_read(b)
    assert (first[2][~odd] == ACTIVE).all() and np.array_equal(first[0][~odd], xy[~odd])
    assert (first[2][odd] == EXITED).sum() >= 300 and not (first[2][odd] == ACTIVE).any()
    for pid in (a, b):
        dev.particles_set_diffusivity(pid, K, seed)
    t = 0.0
    for j in range(10):
        dev.advance(1)
        t += dt_move
        dev.particles_advance_at(a, dt_move, t, open_markers)
        dev.particles_advance_at(b, dt_move, t, open_markers)
    ra, rb = dev.particles_read(a), dev.particles_read(b)
    same_particles([r[~odd] for r in rb], [r[~odd] for r in ra], 'even particles')
    assert np.array_equal(rb[0][odd], first[0][odd]) and not np.array_equal(ra[0][~odd], xy[~odd])
    dev.close()


def test_seeds(hip_lib):
    mesh, dev, dt_move, open_markers = _device('channel')
    xy, cells = random_particles(mesh, 300, seed=3)
    K, _ = walk_scenario('channel', 'constant')
    sets = [_pair(mesh, dev, xy, cells, K, s) for s in (1, 1, 2, 1 + 2**32)]
    _moves(dev, sets, dt_move, open_markers, 2)
    r = [dev.particles_read(pid)[0] for pid, _ in sets]
    assert np.array_equal(r[0], r[1])
    for other in (r[2], r[3]):                                                                # both halves of the seed are the key
        assert (r[0] != other).any(axis=1).mean() > 0.9                                       # (a particle that left in the midpoint move has no walk)
    dev.close()


def test_staggered_releases(hip_lib):
    """releases spread over the moves (and before, on and just after a move's start, and never): the device follows the host, a
    WAITING particle stays at its release point with no hits, and everybody due has moved"""
    mesh, dev, dt_move, open_markers = _device('coast')
    xy, cells = random_particles(mesh, 700, seed=3)
    release = dt_move*np.linspace(-1.0, 11.0, 700)
    release[::50] = dt_move*np.arange(14)                                     # exactly the start of a move
    release[1::50] = np.nextafter(dt_move*np.arange(14), np.inf)              # an ulp later: the next move
    release[5] = np.inf
    K, seed = walk_scenario('coast', 'constant')
    timed, both = _pair(mesh, dev, xy, cells, release=release), _pair(mesh, dev, xy, cells, K, seed, release)
    for pid, host in (timed, both):
        assert np.array_equal(host.status == WAITING, release > 0.0) and (host.status == WAITING).sum() > 600
    t = 0.0
    for j in range(10):
        dev.advance(1)
        t += dt_move
        for pid, host in (timed, both):
            dev.particles_advance_at(pid, dt_move, t, open_markers)
        uv, _ = dev.get_state()
        for pid, host in (timed, both):
            host.advance_at(uv, dt_move, t, open_markers)
            got = dev.particles_read(pid)
            same_particles(got, host.read(), 'move {:d}'.format(j))
            waiting = release > t - dt_move
            assert np.array_equal(got[2] == WAITING, waiting)
            assert np.array_equal(got[0][waiting], xy[waiting]) and (got[4][waiting] == 0).all()
            assert (got[0][~waiting] != xy[~waiting]).any(axis=1).all()
    c = dev.particles_cell_counts(both[0], (WAITING,))
    assert np.array_equal(c, both[1].cell_counts((WAITING,))) and c.sum() == (release > t - dt_move).sum() > 0
    dev.close()


# ---- FlowSolver2d: batches, and which entry point a set goes through
N_STEPS, EVERY, DT = 24, 4, 0.3


def _solver_run(mode, **kw):
    mesh = stats_mesh('triangles')
    s = make_solver(mesh, make_forcing(mesh, K=3), dt=DT, n_steps=N_STEPS, n_export=12)
    xy, _ = random_particles(mesh, 300, seed=12)
    cb = ParticleTrackerCallback(s, xy, every=EVERY, record_every=2, open_boundaries=(1,), export_to_hdf5=False, row_capacity=2, **kw)
    s.add_callback(cb, eval_interval='timestep')
    dev = s.timestepper.device
    calls = {'advance': [], 'old': 0, 'new': []}
    inner, old, new = dev.advance, dev.particles_advance, dev.particles_advance_at
    dev.advance = lambda n=1: (calls['advance'].append(int(n)), inner(n))[1]
    dev.particles_advance = lambda *a, **k: (calls.__setitem__('old', calls['old'] + 1), old(*a, **k))[1]
    dev.particles_advance_at = lambda pid, dt_move, t, open_markers=(): (calls['new'].append(float(t)), new(pid, dt_move, t, open_markers))[1]
    if mode == 'iterate':
        s.iterate()
    else:
        for _ in s.create_iterator():
            pass
    assert s.iteration == N_STEPS
    out = {'calls': calls, 'state': (cb.positions(), cb.cells(), cb.status(), cb.exit_markers(), cb.wall_hits()), 'traj': cb.trajectories(),
           'counts': cb.cell_counts(), 'conc': cb.concentration().dat.data_ro.copy(), 'start': xy, 'areas': mesh.cell_areas()}
    dev.close()
    return out


def test_batched_equals_step_by_step(hip_lib):
    """24 steps, a move every 4th: iterate() sends 6 batches of 4 steps, the loop 24 single steps; with dispersion (steps of about 30
    m in cells of 500 m) and releases staggered over the run the particles, the recorded rows and the counts are the same bits"""
    kw = {'diffusivity': 120.0, 'seed': 77, 'release_times': np.linspace(-1.0, 1.2*N_STEPS*DT, 300)}
    batched, loop = _solver_run('iterate', **kw), _solver_run('loop', **kw)
    assert batched['calls']['advance'] == [EVERY]*(N_STEPS//EVERY) and loop['calls']['advance'] == [1]*N_STEPS
    for r in (batched, loop):
        assert r['calls']['old'] == 0 and np.allclose(r['calls']['new'], EVERY*DT*np.arange(1, 7), rtol=1e-15)
    assert batched['calls']['new'] == loop['calls']['new']
    same_particles(batched['state'], loop['state'], 'iterate() against the loop')
    assert np.array_equal(batched['traj'][0], loop['traj'][0]) and np.array_equal(batched['traj'][1], loop['traj'][1])
    st = batched['state'][2]
    assert (st == WAITING).any() and (st == ACTIVE).any() and batched['traj'][1].shape == (3, 300, 2)
    waiting = st == WAITING
    assert np.array_equal(batched['traj'][1][:, waiting], np.broadcast_to(batched['start'][waiting], (3, int(waiting.sum()), 2)))
    assert np.array_equal(batched['counts'], loop['counts']) and batched['counts'].sum() == (st == ACTIVE).sum()
    assert np.array_equal(batched['counts'], np.bincount(batched['state'][1][st == ACTIVE], minlength=len(batched['counts'])))
    assert np.array_equal(batched['conc'], batched['counts']/batched['areas'])
    plain = _solver_run('iterate')
    assert not np.array_equal(plain['state'][0], batched['state'][0])


def test_a_set_without_the_features_goes_through_the_old_entry_point(hip_lib):
    plain = _solver_run('iterate')
    assert plain['calls']['old'] == N_STEPS//EVERY and plain['calls']['new'] == []
    assert plain['counts'].sum() == (plain['state'][2] == ACTIVE).sum()                      # counting alone does not change the path
    zero = _solver_run('iterate', diffusivity=0.0)
    assert zero['calls']['old'] == 0 and len(zero['calls']['new']) == N_STEPS//EVERY
    same_particles(zero['state'], plain['state'], 'diffusivity 0 against no diffusivity')


# ---- lifecycle
def _code(call):
    with pytest.raises(_lib.Swe2dError) as err:
        call()
    return err.value.code


def test_lifecycle_of_the_new_calls(hip_lib):
    mesh, dev, dt_move, open_markers = _device('channel')
    xy, cells = random_particles(mesh, 9, seed=4)
    pid = dev.particles_create(xy, cells)
    nv = mesh.num_vertices
    bad = np.full(nv, 1.0)
    bad[7] = -1e-300
    for K in (-1.0, float('nan'), float('inf'), bad, np.ones(nv - 1), np.ones(nv + 1)):
        assert _code(lambda: dev.particles_set_diffusivity(pid, K)) == _lib.ERR_INVALID_ARGUMENT
    for r in (np.zeros(8), np.zeros(10), np.full(9, np.nan)):
        assert _code(lambda: dev.particles_set_release_times(pid, r)) == _lib.ERR_INVALID_ARGUMENT
    assert _code(lambda: dev.particles_advance_at(pid, dt_move, float('nan'))) == _lib.ERR_INVALID_ARGUMENT
    assert _code(lambda: dev.particles_advance_at(pid, float('inf'), 0.0)) == _lib.ERR_INVALID_ARGUMENT
    calls = (lambda i: dev.particles_set_diffusivity(i, 1.0, 3), lambda i: dev.particles_set_release_times(i, np.zeros(9)),
             lambda i: dev.particles_advance_at(i, dt_move, dt_move, open_markers), lambda i: dev.particles_cell_counts(i))
    for call in calls:
        for i in (-1, 1, 99):                                                 # a bad id
            assert _code(lambda: call(i)) == _lib.ERR_INVALID_ARGUMENT
    same_particles(dev.particles_read(pid), _host(mesh, xy, cells).read(), 'after the refusals')
    dev.advance(1)
    dev.particles_advance_at(pid, dt_move, dt_move, open_markers)            # a set without either feature: the plain instance
    host = _host(mesh, xy, cells)
    host.advance_at(dev.get_state()[0], dt_move, dt_move, open_markers)
    same_particles(dev.particles_read(pid), host.read(), 'advance_at without features')
    dev.particles_set_diffusivity(pid, 1.0, 3)
    assert _code(lambda: dev.particles_advance_at(pid, -dt_move, 0.0)) == _lib.ERR_INVALID_ARGUMENT   # no walk back in time
    for call in calls:
        call(pid)
    dev.particles_destroy(pid)
    for call in calls:
        assert _code(lambda: call(pid)) == _lib.ERR_INVALID_ARGUMENT
    again = dev.particles_create(xy, cells)                                   # the slot is reused, without the old set's features
    assert again == pid and dev.particles_cell_counts(again).sum() == 9
    dev.close()                                                               # swe2d_destroy with a live set that has all buffers


def test_quadrilaterals_are_unsupported(hip_lib):
    mesh = RectangleMesh(6, 4, 6000.0, 4000.0, quadrilateral=True)
    dev = Swe2dDevice(mesh, np.full(mesh.num_vertices, 10.0), 0.5)
    dev.set_state(np.zeros((mesh.num_cells, 4, 2)), np.zeros((mesh.num_cells, 4)))
    for call in (lambda: dev.particles_set_diffusivity(0, 1.0), lambda: dev.particles_set_release_times(0, [0.0]),
                 lambda: dev.particles_advance_at(0, 1.0, 1.0), lambda: dev.particles_cell_counts(0)):
        assert _code(call) == _lib.ERR_UNSUPPORTED
    dev.advance(1)
    assert np.isfinite(dev.get_state()[1]).all()
    dev.close()


def test_refused_inside_a_stream_capture(hip_lib):
    import torch
    mesh, dev, dt_move, open_markers = _device('channel')
    xy, cells = random_particles(mesh, 9, seed=4)
    pid, host = _pair(mesh, dev, xy, cells, 3.0, 8, np.zeros(9))
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        buf = torch.zeros(16, device='cuda')
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            buf.add_(1.0)                                     # (the capture records something; nothing is replayed)
            for call in (lambda: dev.particles_set_diffusivity(pid, 1.0), lambda: dev.particles_set_release_times(pid, np.ones(9)),
                         lambda: dev.particles_advance_at(pid, dt_move, dt_move, open_markers), lambda: dev.particles_cell_counts(pid)):
                assert _code(call) == _lib.ERR_UNSUPPORTED
        s.synchronize()
        dev.advance(1)                                        # the handle is usable, the set untouched
        dev.particles_advance_at(pid, dt_move, dt_move, open_markers)
        got = dev.particles_read(pid)
    dev.set_stream(None)
    host.advance_at(dev.get_state()[0], dt_move, dt_move, open_markers)
    same_particles(got, host.read(), 'after the capture')
    dev.close()


def test_the_plume_example_runs(hip_lib):
    r = subprocess.run([sys.executable, os.path.join('examples', 'particle_plume.py'), '--periods', '0.05', '--particles', '500'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('concentration maximum')]
    assert len(line) == 1 and float(line[0].split()[2]) > 0.0, r.stdout[-2000:]
    counted = [ln for ln in r.stdout.splitlines() if ln.startswith('particles counted')]
    assert len(counted) == 1 and 0 < int(counted[0].split()[2]) <= 500
