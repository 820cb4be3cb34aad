"""Random-walk dispersion, timed releases and cell counts of the particle tracker on the host (thetis_amd/particles.py): the
generator's known answers, the statistics of the walk in constant and in linearly varying diffusivity, the release gate, the counts,
and the refusals.  tests/test_gpu_particle_walk.py has the device equal to this host path bit for bit."""
import math
import os

import numpy as np
import pytest

from particle_cases import ACTIVE, EXITED, LOST, random_particles, same_particles, scenario
from particle_walk_cases import PHILOX_KNOWN_ANSWERS, bare, deviate_plain, philox_plain, state_of, walk_scenario
from thetis_amd import Constant, Function, get_functionspace, particles
from thetis_amd.mesh import RectangleMesh

WAITING = 3
N, MOVES = 4096, 20


# ---- the generator
def test_philox_known_answers():
    for counter, key, out in PHILOX_KNOWN_ANSWERS:
        assert philox_plain(counter, key) == out
        got = particles.philox4x32_10(np.array(counter), np.array(key))
        assert got.dtype == np.uint32 and tuple(int(w) for w in got) == out
    many = particles.philox4x32_10(np.array([c for c, _, _ in PHILOX_KNOWN_ANSWERS]), np.array([k for _, k, _ in PHILOX_KNOWN_ANSWERS]))
    assert many.tolist() == [list(o) for _, _, o in PHILOX_KNOWN_ANSWERS]


def test_deviates_lie_in_the_half_open_interval_and_follow_the_counter():
    assert deviate_plain(0, 0) == -1.0 and deviate_plain(0xffffffff, 0xffffffff) == 1.0 - 2.0**-52
    seed = 0x123456789abcdef0
    idx = np.arange(100000)
    rx, ry = particles.deviates(seed, idx, 7)
    assert rx.min() >= -1.0 and rx.max() < 1.0 and ry.min() >= -1.0 and ry.max() < 1.0
    assert abs(rx.mean()) < 5/math.sqrt(3*len(idx)) and abs(ry.var() - 1/3) < 0.01            # uniform: variance 1/3
    for p in (0, 1, 4095, 99999):                                                             # counter (index, move, 0, 0), key (low, high)
        w = philox_plain((p, 7, 0, 0), (seed & 0xffffffff, seed >> 32))
        assert (rx[p], ry[p]) == (deviate_plain(w[0], w[1]), deviate_plain(w[2], w[3]))
    assert np.array_equal(particles.deviates(seed, idx[5:9], 7)[0], rx[5:9])                  # whatever the company
    assert not np.array_equal(particles.deviates(seed, idx, 8)[0], rx) and not np.array_equal(particles.deviates(seed + 1, idx, 7)[0], rx)


# ---- the statistics of the walk
def _cloud(mesh, point, diffusivity, dt, seed, n_moves=MOVES):
    rel = np.tile(np.asarray(point, dtype=np.float64), (N, 1))
    cb, step, _ = bare(mesh, np.zeros((mesh.num_cells, 3, 2)), dt, rel, diffusivity=diffusivity, seed=seed)
    step(n_moves)
    return cb, cb.positions() - rel


def test_variance_in_constant_diffusivity():
    """K = 1 m2/s, dt = 60 s on 1000 m x 1000 m (cells of 100 m), 4096 particles from (503, 497): a step is at most sqrt(6 K dt) =
    19 m per coordinate, 20 of them 379 m < 497 m, so no particle can reach a boundary.  The variance of each coordinate is
    20 * 2 K dt = 2400 m2 within 11 % (5 standard errors of sqrt((2 - 1.2/20)/4096) = 2.2 %), the mean within 5 sigma/64 = 3.83 m.
    Seed 2024 gives: variance (2440.8, 2415.9) m2 (+1.7 %, +0.7 %), mean (0.187, 0.338) m."""
    K, dt = 1.0, 60.0
    assert MOVES*math.sqrt(6*K*dt) < 497.0
    cb, d = _cloud(RectangleMesh(10, 10, 1000.0, 1000.0), (503.0, 497.0), K, dt, seed=2024)
    assert (cb.wall_hits() == 0).all() and (cb.status() == ACTIVE).all()
    want = MOVES*2*K*dt
    var, mean = d.var(axis=0), d.mean(axis=0)
    print('variance', var, 'of', want, 'mean', mean)
    assert np.abs(var/want - 1.0).max() <= 5*math.sqrt((2 - 1.2/MOVES)/N)
    assert np.abs(mean).max() <= 5*math.sqrt(want)/64
    assert len(set(cb.cells().tolist())) > 10                                                 # through many cells
    again, d2 = _cloud(RectangleMesh(10, 10, 1000.0, 1000.0), (503.0, 497.0), Constant(K), dt, seed=2024)
    assert np.array_equal(d, d2)                                                              # deterministic for a seed
    assert np.allclose(var, [2440.8, 2415.9], rtol=1e-4) and np.allclose(mean, [0.187, 0.338], atol=1e-3)


def test_drift_in_linear_diffusivity():
    """K = g x (CG-P1, zero at the wall x = 0), particles from x = 400 m: every step has the mean g dt whatever its start, so the
    mean displacement after n = 20 moves is D = n g dt, here 280 m.  Its variance is the sum of the steps' 2 dt Ko = 2 dt K(x_j) +
    (g dt)^2 with E K(x_j) = g (400 + j g dt): sigma^2 = 2 n dt g 400 + D^2, sigma = 549.9 m, D = 0.509 sigma = 32.6 standard errors
    of the mean (sigma/64); 5 are allowed.  (D >= sigma/2 and K >= 0 on the mesh force D >= 2/3 of the distance to the wall where
    K vanishes: the cloud reaches that wall, where a step is cut short and stops being exact.  Seed 7: 4096 particles count about
    300 such hits in 81920 steps, each shortening one step of a few g dt = 14 m; the mean comes out at -1.5 standard errors.)"""
    n, dt, x0 = MOVES, 60.0, 400.0
    D = 0.7*x0
    g = D/(n*dt)
    mesh = RectangleMesh(20, 20, 4000.0, 8000.0)
    K = Function(get_functionspace(mesh, 'CG', 1)).interpolate(lambda x, y: g*x)
    sigma = math.sqrt(2*n*dt*g*x0 + D*D)
    assert D >= 0.5*sigma
    cb, d = _cloud(mesh, (x0, 4003.0), K, dt, seed=7)
    assert not np.isin(cb.status(), (EXITED, LOST)).any()
    print('drift', d[:, 0].mean(), 'of', D, 'in standard errors', (d[:, 0].mean() - D)/(sigma/64), 'wall hits', int(cb.wall_hits().sum()))
    # without the dt*g term in the displacement the mean stays near 0, 32 standard errors off: this assertion fails
    assert abs(d[:, 0].mean() - D) <= 5*sigma/64
    assert abs(d[:, 1].mean()) <= 5*d[:, 1].std()/64                                          # and none across the gradient


# ---- opt-in means opt-in
@pytest.mark.parametrize('case', ['channel', 'coast'])
def test_zero_diffusivity_changes_nothing(case):
    mesh, _, uv, _, _, dt, open_markers = scenario(case)
    xy, _ = random_particles(mesh, 300, seed=3)
    plain, step_p, _ = bare(mesh, uv, dt, xy, open_boundaries=open_markers)
    zero, step_z, _ = bare(mesh, uv, dt, xy, open_boundaries=open_markers, diffusivity=0.0, seed=99)
    for j in range(10):
        step_p()
        step_z()
        same_particles(state_of(zero), state_of(plain), 'move {:d}'.format(j))
    assert plain.wall_hits().sum() > 0 and (plain.status() == EXITED).any()
    assert plain._host.n_moves == 0 and zero._host.n_moves == 10                              # the old entry point, the new one


def test_walk_meets_walls_exits_and_the_hop_cap():
    """the scenarios of the GPU test do on the host what they claim: the second walk alone ends at walls, exits and, with moves of
    many cells, at the hop cap"""
    mesh, _, uv, _, _, dt, open_markers = scenario('channel')
    xy, _ = random_particles(mesh, 700, seed=3)
    K, seed = walk_scenario('channel', 'strong')
    cb, step, _ = bare(mesh, 0.0*uv, dt, xy, open_boundaries=open_markers, diffusivity=K, seed=seed)
    step(3)
    assert cb.wall_hits().sum() > 0 and (cb.status() == EXITED).any() and not (cb.status() == LOST).any()
    mesh, _, uv, _, _, dt, open_markers = scenario('cap')
    xy, _ = random_particles(mesh, 700, seed=3)
    cb, step, _ = bare(mesh, 0.0*uv, 1200.0, xy, open_boundaries=open_markers, diffusivity=2.0e6, seed=5)
    step(1)
    lost = cb.status() == LOST
    assert lost.any() and np.array_equal(cb.positions()[lost], xy[lost]) and (cb.wall_hits()[lost] == 0).all()


# ---- timed releases
def test_release_times_gate_the_moves():
    """dt = 1200 s, moves at t = 1200 j that start at 1200 (j - 1): a particle released at t_r first moves in move 1 + ceil(t_r/1200).
    Before that it is WAITING at its release point in every row; from then on it does what a particle that was ACTIVE from the
    start does when it is advanced by those moves only (frozen velocity: the moves are the same)."""
    mesh, _, uv, _, _, dt, open_markers = scenario('channel')
    xy, _ = random_particles(mesh, 60, seed=6)
    t_r = np.repeat([-1.0, 0.0, 1.0, 1200.0, 1200.5, 4800.0, 1e9, np.inf, -np.inf, 3599.9999], 6)
    first = np.array([1 if t <= 0 else 10**6 if t > 1e8 else 1 + math.ceil(t/dt) for t in t_r])   # the first move that moves it (1-based)
    cb, step, _ = bare(mesh, uv, dt, xy, open_boundaries=open_markers, release_times=t_r)
    assert np.array_equal(cb.status() == WAITING, t_r > 0.0) and np.array_equal(cb.positions(), xy)
    n_moves = 8
    twins = {}
    for j in range(1, n_moves + 1):
        twins[j] = bare(mesh, uv, dt, xy, open_boundaries=open_markers)                     # starts with move j
        step()
        for j0, (twin, twin_step, _) in twins.items():
            twin_step()
        waiting = first > j
        assert np.array_equal(cb.status() == WAITING, waiting)
        assert np.array_equal(cb.positions()[waiting], xy[waiting]) and (cb.wall_hits()[waiting] == 0).all()
        for j0, (twin, _, _) in twins.items():
            sel = first == j0
            same_particles([a[sel] for a in state_of(cb)], [a[sel] for a in state_of(twin)], 'released in move {:d}, after move {:d}'.format(j0, j))
    t, rows = cb.trajectories()
    assert rows.shape == (n_moves, 60, 2)
    for j in range(n_moves):
        assert np.array_equal(rows[j][first > j + 1], xy[first > j + 1])                    # rows show WAITING particles at their release point
    assert (first > n_moves).sum() == 12 and not np.array_equal(rows[-1][first == 1], xy[first == 1])


# ---- cell counts
def test_cell_counts_and_concentration():
    mesh, _, uv, _, _, dt, open_markers = scenario('channel')
    xy, _ = random_particles(mesh, 700, seed=3)
    t_r = np.where(np.arange(700) % 7 == 0, 1e9, 0.0)
    cb, step, _ = bare(mesh, uv, dt, xy, open_boundaries=open_markers, release_times=t_r, diffusivity=50.0)
    before = cb.cell_counts()                                                                 # no set yet
    assert before.sum() == 600 and before.dtype == np.int32
    step(6)
    st, cells = cb.status(), cb.cells()
    assert (st == EXITED).any() and (st == WAITING).sum() == 100
    for status in ((ACTIVE,), (EXITED,), (WAITING,), (ACTIVE, WAITING), (ACTIVE, EXITED, LOST, WAITING)):
        c = cb.cell_counts(status)
        sel = np.isin(st, status)
        assert c.shape == (mesh.num_cells,) and c.dtype == np.int32 and c.sum() == sel.sum()
        assert np.array_equal(c, np.bincount(cells[sel], minlength=mesh.num_cells))
    conc = cb.concentration()
    fs = conc.function_space()
    assert (fs.family, fs.degree) == ('DG', 0) and np.array_equal(conc.dat.data_ro, cb.cell_counts()/mesh.cell_areas())
    # a permuted particle order: the same counts
    perm = np.random.default_rng(1).permutation(700)
    host = cb._host
    other = particles.HostParticles(mesh.cells, mesh.vertex_xy, mesh.cell_nbr, mesh.cell_nbr_facet, host.xy[perm], host.cell[perm])
    other.status[:] = host.status[perm]
    assert np.array_equal(other.cell_counts((ACTIVE,)), cb.cell_counts())


def test_export_carries_the_new_fields(tmp_path):
    mesh, _, uv, _, _, dt, open_markers = scenario('channel')
    xy, _ = random_particles(mesh, 5, seed=3)
    cb, step, _ = bare(mesh, uv, dt, xy, release_times=np.arange(5.0), diffusivity=2.0, seed=2**63 + 5)
    cb.export_to_hdf5, cb.outputdir = True, str(tmp_path)
    step(2)
    cb.export()
    d = np.load(os.path.join(str(tmp_path), 'diagnostic_particles.npz'))
    assert np.array_equal(d['release_times'], np.arange(5.0)) and int(d['seed']) == 2**63 + 5
    assert np.array_equal(d['diffusivity'], np.full(mesh.num_vertices, 2.0))


# ---- refusals
def test_bad_arguments_are_refused():
    mesh, _, uv, _, _, dt, _ = scenario('channel')
    xy, _ = random_particles(mesh, 4, seed=3)
    nv = mesh.num_vertices
    neg = np.full(nv, 1.0)
    neg[3] = -1e-9
    for K in (-1.0, Constant(-0.5), float('nan'), float('inf'), neg, np.ones(nv - 1), np.ones((nv, 2))):
        with pytest.raises(ValueError):
            bare(mesh, uv, dt, xy, diffusivity=K)
    negf = Function(get_functionspace(mesh, 'CG', 1))
    negf.dat.data[5] = -2.0
    with pytest.raises(ValueError):
        bare(mesh, uv, dt, xy, diffusivity=negf)
    for fs in (get_functionspace(mesh, 'DG', 1), get_functionspace(mesh, 'DG', 0), get_functionspace(mesh, 'CG', 1, vector=True)):
        with pytest.raises(NotImplementedError, match='kdiff'):
            bare(mesh, uv, dt, xy, diffusivity=Function(fs, name='kdiff'))
    for r in (np.zeros(3), np.zeros((4, 2)), [0.0, 1.0, float('nan'), 2.0]):
        with pytest.raises(ValueError):
            bare(mesh, uv, dt, xy, release_times=r)
    with pytest.raises(ValueError):
        bare(mesh, uv, dt, xy, diffusivity=1.0, seed=-1)
    host = particles.HostParticles(mesh.cells, mesh.vertex_xy, mesh.cell_nbr, mesh.cell_nbr_facet, xy, bare(mesh, uv, dt, xy)[0].initial_cells)
    with pytest.raises(ValueError):
        host.set_diffusivity(np.ones(nv + 1))
    with pytest.raises(ValueError):
        host.set_release_times(np.zeros(5))
    host.set_diffusivity(1.0)
    with pytest.raises(ValueError):
        host.advance_at(uv, -1.0, 0.0)


def test_quadrilaterals_and_several_ranks_still_raise():
    quad = RectangleMesh(4, 3, 1000.0, 400.0, quadrilateral=True)
    with pytest.raises(NotImplementedError, match='triangles'):
        bare(quad, np.zeros((quad.num_cells, 4, 2)), 10.0, [(10.0, 10.0)], diffusivity=1.0, release_times=[0.0])
    mesh, _, uv, _, _, dt, _ = scenario('channel')
    cb, step, _ = bare(mesh, uv, dt, random_particles(mesh, 2, seed=1)[0], diffusivity=1.0)
    cb.solver_obj.comm.size = 2
    with pytest.raises(NotImplementedError, match='several ranks'):
        step()
