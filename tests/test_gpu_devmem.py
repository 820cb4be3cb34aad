"""Who owns the handle's device memory (thetis_amd/csrc/swe2d_devmem.h), seen through swe2d_debug_live_device_memory: the live bytes and
live allocations of the library, process-wide, as exact integers.

Ownership does not depend on the size of a mesh, so the meshes are the smallest on which every feature can be enabled: 6 x 5 squares
cut into 60 triangles (one partial wave) and 5 x 4 quadrilaterals.  The sediment models, the Smagorinsky closure, the particles,
the discrete farms and the sections do not go with wetting-drying or quadrilaterals: the triangle device takes every owner but the
wetting-drying alpha, the quadrilateral device takes wetting-drying and what goes with it.  Every call is a documented
entry point with valid data, or one with an argument the library rejects on the host."""
import ctypes
import itertools

import numpy as np
import pytest

import discrete_turbine_ref as dr
from bedload_cases import ALPHA_SECC, BETA, SURBETA2
from slide_cases import slide_c
from thetis_amd import Function, RectangleMesh, _lib, get_functionspace, reactions
from thetis_amd.cgproject import elem_size_p1
from thetis_amd.device import Swe2dDevice
from thetis_amd.sediment_model import (bedload_constants, bedload_device_parameters, device_parameters,
                                       slide_device_parameters)

pytestmark = pytest.mark.gpu

LX, LY, DT = 6e3, 5e3, 0.05
OMEGA = 1.4e-4


def live(lib):
    out = (ctypes.c_uint64*2)()
    assert lib.swe2d_debug_live_device_memory(out) == 0
    return int(out[0]), int(out[1])


def _mesh(quadrilateral=False):
    return RectangleMesh(5, 4, LX, LY, quadrilateral=True) if quadrilateral else RectangleMesh(6, 5, LX, LY)


def _device(mesh, seed=0):
    rng = np.random.default_rng(seed)
    n, npc = mesh.cells.shape
    bath = 20.0 + rng.uniform(-0.5, 0.5, size=mesh.num_vertices)
    dev = Swe2dDevice(mesh, bath, DT)
    dev.set_state(1e-2*rng.uniform(-1, 1, size=(n, npc, 2)), 1e-2*rng.uniform(-1, 1, size=(n, npc)))
    return dev


def _constants():
    return bedload_constants(slide_c(), BETA, SURBETA2, ALPHA_SECC, True, True, False)


def _turbine_params(projected_diameter):
    p = _lib.TurbineParams()
    p.rotor_area = np.pi*30.0**2
    p.projected_diameter = projected_diameter
    p.thrust_area_const = 0.8*p.rotor_area
    p.power_const = 0.4
    p.rho0 = 1000.0
    return p


# ---- the setters, one per optional owner: each may be called again with data of the same size
def viscosity(dev, mesh):
    dev.set_viscosity(np.linspace(1.0, 2.0, mesh.num_vertices))


def tracer_extras(dev, mesh, tid=0):
    n, npc = mesh.cells.shape
    dev.tracer_set_source(tid, np.full((n, npc), 1e-3))
    dev.tracer_set_diffusivity(tid, np.linspace(0.5, 1.0, mesh.num_vertices))
    slot = dev._slot(1)
    dev.tracer_set_bc_facets(tid, slot, np.ones((len(dev.boundary_facets(slot)[0]), npc)))


def reaction(dev, mesh, tid=1):
    npc = mesh.cells.shape[1]
    a = Function(get_functionspace(mesh, 'DG', 1))
    p = reactions.compile_source(-0.05*a, lambda f: tid if f is a else None, npc=npc)
    dev.reaction_set_field(0, np.ones(mesh.cells.shape))
    dev.tracer_set_reaction(tid, p.code, p.constant_values(), p.phi, p.w)


def sediment(dev, mesh, tid=2, equilibrium=True):
    dev.sediment_set(tid, device_parameters(_constants(), False, False))
    if equilibrium:
        dev.sediment_set_equilibrium_bc(1)            # (its value planes are the tracer's and stay with it)


def bedload(dev, mesh):
    dev.bedload_set(bedload_device_parameters(_constants(), False), [2])


def slide(dev, mesh):
    dev.slide_set(slide_device_parameters(_constants(), False), np.ones(mesh.num_cells))


def smagorinsky(dev, mesh):
    dev.smag_set(0.1, elem_size_p1(mesh))
    dev.smag_read('gradient')                                 # (the debug planes are allocated by the first read)


def continuous_farm(dev, mesh):
    n, npc = mesh.cells.shape
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    dev.turbine_farm_set(0, _turbine_params(18.0), np.where((xc < 4e3)[:, None], 1e-5, 0.0)*np.ones((1, npc)))


def discrete_farm(dev, mesh):
    phi, w = dr.rule(mesh.cells.shape[1], 4)
    dev.dfarm_set(1, _turbine_params(1.5e3), [[2e3, 2e3], [3e3, 2.5e3], [0.2e3, 4e3]], np.ones(mesh.num_cells, dtype=bool), phi, w)


def power_rows(dev, mesh, capacity=2):
    dev.turbine_rows_reserve(capacity)


def tide(dev, mesh, K=2):
    slot = dev._slot(1)
    n = len(dev.boundary_facets(slot)[0])
    dev.tide_set([slot], OMEGA*np.arange(1, K + 1), np.zeros((n, 2)), 0.1*np.ones((K, n, 2)), np.zeros((K, n, 2)))


def atmosphere(dev, mesh, n_t=3):
    nv = mesh.num_vertices
    dev.atm_set(np.arange(n_t)*100.0, wind_u=np.full((n_t, nv), 5.0), wind_v=np.zeros((n_t, nv)), pressure=np.full((n_t, nv), 1e5))


def sections(dev, mesh, tids=()):
    npc = mesh.cells.shape[1]
    w = np.full((2, 2, npc), 1.0/npc)
    dev.sections_set(2, [0, 1], [3, 7], w, [[0.0, 50.0], [50.0, 0.0]], tracer_ids=tids)
    dev.sections_rows_reserve(2)


def snapshots(dev, mesh):
    dev.snapshot(0)
    dev.snapshot(1)


def probes(dev, mesh, capacity=2, tracer=False):
    npc = mesh.cells.shape[1]
    return dev.probe_create([0, 5, 11], np.full((3, npc), 1.0/npc), ['uv', 'elev'] + ([0] if tracer else []), capacity=capacity)


def statistics(dev, mesh):
    return dev.stats_create(1)


def particles(dev, mesh, full=True):
    xy = mesh.cell_xy()[[2, 9, 30]].mean(axis=1)
    pid = dev.particles_create(xy, [2, 9, 30], capacity=2)
    if full:
        dev.particles_set_diffusivity(pid, 0.5, seed=3)
        dev.particles_set_release_times(pid, [0.0, 0.0, 1.0])
        dev.particles_cell_counts(pid)
    return pid


def _everything_on_triangles(dev, mesh):
    for tid in range(3):
        assert dev.add_tracer() == tid
        dev.tracer_set_state(tid, np.full(mesh.cells.shape, 0.5))
    viscosity(dev, mesh)
    tracer_extras(dev, mesh)
    reaction(dev, mesh)
    sediment(dev, mesh)
    bedload(dev, mesh)
    slide(dev, mesh)
    smagorinsky(dev, mesh)
    probes(dev, mesh, tracer=True)
    continuous_farm(dev, mesh)
    discrete_farm(dev, mesh)
    power_rows(dev, mesh)
    tide(dev, mesh)
    atmosphere(dev, mesh)
    statistics(dev, mesh)
    particles(dev, mesh)
    sections(dev, mesh, tids=[0])
    snapshots(dev, mesh)


def _everything_on_quadrilaterals(dev, mesh):
    assert dev.add_tracer() == 0
    dev.tracer_set_state(0, np.full(mesh.cells.shape, 0.5))
    dev.set_wetting_and_drying(np.full(mesh.num_vertices, 0.5))
    viscosity(dev, mesh)
    tracer_extras(dev, mesh)
    probes(dev, mesh, tracer=True)
    continuous_farm(dev, mesh)
    power_rows(dev, mesh)
    tide(dev, mesh)
    atmosphere(dev, mesh)
    statistics(dev, mesh)
    snapshots(dev, mesh)


@pytest.mark.parametrize('quadrilateral', [False, True], ids=['triangles', 'quadrilaterals'])
def test_destroy_returns_everything(hip_lib, quadrilateral):
    mesh = _mesh(quadrilateral)
    start = live(hip_lib)
    for _ in range(3):
        dev = _device(mesh)
        (_everything_on_quadrilaterals if quadrilateral else _everything_on_triangles)(dev, mesh)
        assert live(hip_lib)[1] > start[1]
        dev.tide_clock(0.0)
        dev.advance_coupled(2)
        dev.synchronize()
        dev.close()
        assert live(hip_lib) == start


def test_setting_twice_does_not_grow(hip_lib):
    mesh = _mesh()
    start = live(hip_lib)
    dev = _device(mesh)
    for tid in range(3):
        dev.add_tracer()
    setters = [viscosity, tracer_extras, reaction, sediment, bedload, slide, smagorinsky, continuous_farm, discrete_farm, power_rows,
               tide, atmosphere, sections, snapshots]
    for setter in setters:
        setter(dev, mesh)
        first = live(hip_lib)
        setter(dev, mesh)
        assert live(hip_lib) == first, setter.__name__
    # data of another size, then the first size again
    for setter, other in ((tide, dict(K=3)), (atmosphere, dict(n_t=5)), (power_rows, dict(capacity=7))):
        setter(dev, mesh)
        first = live(hip_lib)
        setter(dev, mesh, **other)
        assert live(hip_lib)[0] > first[0], setter.__name__
        setter(dev, mesh)
        assert live(hip_lib) == first, setter.__name__
    # the sets with ids: a destroyed set gives everything back, the next one of the same size takes as much again
    for create, destroy, other in ((probes, dev.probe_destroy, dict(capacity=9)), (statistics, dev.stats_destroy, None),
                                   (particles, dev.particles_destroy, dict(full=False))):
        before = live(hip_lib)
        sid = create(dev, mesh)
        first = live(hip_lib)
        destroy(sid)
        assert live(hip_lib) == before, create.__name__
        if other is not None:
            sid = create(dev, mesh, **other)
            assert live(hip_lib) != first, create.__name__
            destroy(sid)
        assert create(dev, mesh) == sid
        assert live(hip_lib) == first, create.__name__
    dev.close()
    assert live(hip_lib) == start


def test_shared_sediment_tables_have_one_owner(hip_lib):
    mesh = _mesh()
    start = live(hip_lib)
    dev = _device(mesh)
    assert dev.add_tracer() == 0
    dev.tracer_set_state(0, np.full(mesh.cells.shape, 0.5))
    on = {'sediment': lambda: sediment(dev, mesh, 0, equilibrium=False), 'bedload': lambda: bedload(dev, mesh), 'slide': lambda: slide(dev, mesh)}
    off = {'sediment': dev.sediment_clear, 'bedload': dev.bedload_clear, 'slide': dev.slide_clear}
    # what a first step builds for good (limiter tables, tile tables) is there before the reading that the orders come back to
    for name in sorted(on):
        on[name]()
    dev.exner_step()
    dev.advance_coupled(1)
    for name in sorted(on):
        off[name]()
        dev.advance_coupled(1)
    dev.synchronize()
    before = live(hip_lib)
    for order in itertools.permutations(sorted(on)):
        for name in sorted(on):
            on[name]()
        full = live(hip_lib)
        for i, name in enumerate(order):
            off[name]()
            if i < 2:                                         # the remaining models still have their tables
                assert before[1] < live(hip_lib)[1] < full[1], order
                dev.exner_step()
                dev.advance_coupled(1)
                dev.synchronize()
        assert live(hip_lib) == before, order
    dev.close()
    assert live(hip_lib) == start


def test_a_rejected_creation_leaves_nothing(hip_lib):
    mesh = _mesh()
    dev = _device(mesh)
    before = live(hip_lib)
    npc = mesh.cells.shape[1]
    with pytest.raises(_lib.Swe2dError):
        dev.probe_create([0, 1], np.full((2, npc), 1.0/npc), ['uv'], capacity=-1)
    # (the cell of a probe as the library itself checks it, past Swe2dDevice's renumbering)
    cells, pid = np.array([0, mesh.num_cells], dtype=np.int32), ctypes.c_int32()
    w, fields = np.full((2, npc), 1.0/npc), np.array([_lib.PROBE_UV], dtype=np.int32)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert hip_lib.swe2d_probe_create(dev.h, 2, cells.ctypes.data_as(ip), w.ctypes.data_as(dp), 1, fields.ctypes.data_as(ip), 0,
                                      ctypes.byref(pid)) == _lib.ERR_INVALID_ARGUMENT
    xy = np.ascontiguousarray(mesh.cell_xy()[[2, 9]].mean(axis=1))
    with pytest.raises(_lib.Swe2dError):
        dev.particles_create(xy, [2, 9], capacity=-1)
    # (Swe2dDevice.particles_create refuses a cell out of range itself: the library's own check, asked directly)
    cells = np.array([2, mesh.num_cells], dtype=np.int32)
    assert hip_lib.swe2d_particles_create(dev.h, 2, xy.ctypes.data_as(dp), cells.ctypes.data_as(ip), 0,
                                          ctypes.byref(pid)) == _lib.ERR_INVALID_ARGUMENT
    assert live(hip_lib) == before
    dev.close()
