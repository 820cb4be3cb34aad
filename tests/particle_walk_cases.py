"""Shared helpers of the random-walk, timed-release and cell-count tests of the particle tracker (tests/test_particle_walk.py on the
CPU, tests/test_gpu_particle_walk.py on the GPU): a callback on a solver stand-in without a device, an independent Philox4x32-10 in
plain Python integers, the diffusivity fields and the scenarios both files run."""
import types

import numpy as np

from thetis_amd import ParticleTrackerCallback

PHILOX_KNOWN_ANSWERS = [      # (counter, key, output): 32-bit words
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,)*4, (0xffffffff,)*2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox_plain(counter, key):
    """Philox4x32-10 in Python integers, written from the specification (not imported from thetis_amd/particles.py)"""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53*c[0], 0xCD9E8D57*c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


def deviate_plain(wa, wb):
    return 2.0*(((wa >> 5)*67108864.0 + (wb >> 6))*2.0**-53) - 1.0


def bare(mesh, uv, dt, positions, **kw):
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


def state_of(cb):
    return cb.positions(), cb.cells(), cb.status(), cb.exit_markers(), cb.wall_hits()


def varying_diffusivity(mesh, k_mean):
    """a per-vertex table that varies over the mesh by a factor of about three: k_mean*(1 + 0.5 sin + 0.3 cos) > 0"""
    x, y = mesh.vertex_xy.T
    lx, ly = np.ptp(x), np.ptp(y)
    return k_mean*(1.0 + 0.5*np.sin(5.0*(x - x.min())/lx) + 0.3*np.cos(7.0*(y - y.min())/ly))


def walk_scenario(name, kind):
    """(diffusivity, seed) for the scenario ``name`` of particle_cases ('channel': cells of 5 km x 3.8 km, dt_move 1200 s; 'coast':
    dt_move 450 s).  ``kind``: 'constant' and 'varying' (steps of about a fifth of a cell), 'strong' (steps of up to three cells: walls and exits in the second walk)"""
    from particle_cases import scenario
    mesh, _, _, _, _, dt_move, _ = scenario(name)
    size = float(np.sqrt(mesh.cell_areas().mean()))
    frac = {'constant': 0.2, 'varying': 0.2, 'strong': 3.0}[kind]
    k_mean = (frac*size)**2/(6.0*dt_move)                      # sqrt(6 K dt) = frac * cell size
    if kind == 'constant':
        return k_mean, 11
    return varying_diffusivity(mesh, k_mean), 2**40 + 12345
