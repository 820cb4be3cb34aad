"""
Discrete tidal turbine farms on the device (csrc/swe2d_dfarm.hip) against tests/discrete_turbine_ref.py: the tabulated bump density,
the drag pass' share of a tendency, stepping, the ends of the cell lists, the power per farm and per turbine, the batched time loop,
the slot's lifecycle and the example.

Tolerances.  Density: 8 eps of the peak 1/(r^2 1.45661) times the largest number of overlapping bumps (the bump's sensitivity to the
rounding of 1/(1 - s^2) is at most ~1.5 eps of the peak - max t^2 e^(1-t) = 4/e - plus a couple of ulp of the two exp routines; the
points are the same doubles on both sides, formed left to right without contraction).  TOL_RHS = 1e-12 relative L-infinity of the
FULL tendency for the farm's share, 1e-11 after 20 steps, 1e-13 relative for the power, (n_turbines + 2) eps relative between a
farm's power and the sum of its turbines' (both are exact sums of terms that differ by their roundings).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import discrete_turbine_ref as dr
import turbine_ref as tr
from helpers import channel_case, make_oracle, make_oracle_generic, quad_case, rel_linf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
TOL_RHS = 1e-12
SPEEDS = [0.9, 1., 3., 5., 5.001]
C_T = [0.01, 0.7, 0.7, 0.1, 0.0001]
R = 8e3                                                          # bump radius: about two cells of the 24 x 8 meshes
# one interior | two overlapping | across the domain boundary | across the subdomain's edge (x_c < 70 km) | above the upper left corner
# of the domain, its square 1 m into column 1 and row 6 of the 24 x 8 grid: the cell there is clipped at a corner only | wholly outside
COORDS = [[30e3, 15e3], [50e3, 12e3], [54e3, 16e3], [20e3, 1e3], [70e3, 15e3], [100e3/24 + 1.0 - R, 7*30e3/8 - 1.0 + R], [150e3, 15e3]]


def _device(mesh, bath, dt, **kw):
    from thetis_amd.device import Swe2dDevice
    return Swe2dDevice(mesh, bath, dt, **kw)


def _case(kind, seed=0, amp_u=1.0, nx=24, ny=8, lx=100e3):
    if kind == 'tri':
        mesh, bath, uv, eta = channel_case(nx, ny, lx=lx, seed=seed, amp_u=amp_u)
        orc_of = make_oracle
    else:
        mesh, bath, uv, eta = quad_case(nx, ny, lx=lx, seed=seed, amp_u=amp_u, warp=0.2 if kind == 'quad_general' else 0.0)
        orc_of = make_oracle_generic
    return mesh, bath + 20.0, uv, 0.3*eta, orc_of


def _farm(mesh, coords=COORDS, degree=10, edge=70e3, **kw):
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    f = dict(diameter=60.0, projected_diameter=2*R, thrust=0.8, coordinates=np.array(coords, dtype=float).reshape(-1, 2),
             cells=xc < edge, degree=degree)
    f.update(kw)
    return f


def _table_farm(mesh, **kw):
    f = _farm(mesh, upwind=True, C_support=0.6, A_support=10.0, speeds=SPEEDS, thrust_table=C_T, **kw)
    del f['thrust']
    return f


def _params(farm):
    from thetis_amd import _lib
    p = _lib.TurbineParams()
    p.support_area = farm.get('C_support', 0.0)*farm.get('A_support', 0.0)
    p.rotor_area = tr.rotor_area(farm)
    p.projected_diameter = farm.get('projected_diameter') or farm['diameter']
    p.upwind_correction = int(farm.get('upwind', False))
    p.rho0 = 1000.0
    if 'speeds' in farm:
        p.n_table = len(farm['speeds'])
        cp = farm.get('power_table') or [tr.default_power_coefficient(c) for c in farm['thrust_table']]
        for j in range(p.n_table):
            p.speeds[j], p.thrust[j], p.power[j] = farm['speeds'][j], farm['thrust_table'][j], cp[j]
    else:
        p.thrust_area_const = farm['thrust']*tr.rotor_area(farm)
        p.power_const = farm.get('power') or tr.default_power_coefficient(farm['thrust'])
    return p


def _set(dev, slot, farm, npc):
    phi, w = dr.rule(npc, farm['degree'])
    dev.dfarm_set(slot, _params(farm), farm['coordinates'], farm['cells'], phi, w)


def _scaled(uv, mesh, seed=5):
    """speeds from below the table's cut-in to above its cut-out, cell by cell"""
    scale = np.random.default_rng(seed).choice([0.2, 0.95, 2.0, 4.0, 5.0005/1.4, 8.0], size=mesh.num_cells)
    return uv*scale[:, None, None]


# ---- 1. the density table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
@pytest.mark.parametrize('degree', [3, 10, 14])
def test_density_table(hip_lib, kind, degree):
    mesh, bath, uv, eta, orc_of = _case(kind)
    npc = mesh.cells.shape[1]
    farm = _farm(mesh, degree=degree)
    orc = orc_of(mesh, bath)
    dev = _device(mesh, bath, 3.0)
    _set(dev, 2, farm, npc)
    cells, dens = dev.dfarm_density_read(2)
    phi, _ = dr.rule(npc, degree)
    ref = dr.farm_density(orc, farm, phi)                          # (N, q)
    pts = dr.points(orc.p, phi)
    r = dr.radius(farm)
    overlap = sum(((np.abs(pts[..., 0] - x) < r) & (np.abs(pts[..., 1] - y) < r)).astype(int) for x, y in farm['coordinates']).max()
    peak = overlap/(r*r*dr.BUMP_NORM)
    assert dens.shape == (len(phi), len(cells)) and len(set(cells)) == len(cells) and farm['cells'][cells].all()
    listed = np.zeros(mesh.num_cells, dtype=bool)
    listed[cells] = True
    assert not ref[~listed].any()                                  # every cell with a bump at one of its points is listed
    err = np.abs(dens.T - ref[cells]).max()
    print('density table', kind, degree, 'cells', len(cells), 'overlap', overlap, 'max error / peak', err/peak, 'in eps', err/peak/EPS)
    assert overlap >= 2 and err <= 8*EPS*peak
    # the scenario holds what it names: cells cut by the subdomain's edge, the corner cell with no bump at any point, the turbine outside
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    assert (dr.density(dict(farm, coordinates=[COORDS[4]]), pts)[xc >= 70e3] > 0).any() and not ref[xc >= 70e3].any()
    assert kind == 'quad_general' or (~ref[cells].any(axis=1)).any()   # (moved vertices: the 1 m clip is not the grid's)
    assert not dr.density(dict(farm, coordinates=[COORDS[6]]), pts).any()
    dev.close()


# ---- 2. the drag pass' share of a tendency ------------------------------------------------------------------------------------
def _share_check(kind, farms_d, farms_c=(), visc=False, mesh_kw=None, label=''):
    """tendency with the farms minus tendency without, against M^-1 dt R of the reference statements"""
    mesh, bath, uv, eta, orc_of = _case(kind, seed=3, **(mesh_kw or {}))
    npc = mesh.cells.shape[1]
    uv = _scaled(uv, mesh)
    farms_d = [f(mesh) for f in farms_d]
    farms_c = [f(mesh) for f in farms_c]
    orc = orc_of(mesh, bath)
    H = orc.nodal_depth(eta)
    for f in farms_d + farms_c:
        if f.get('upwind'):                                        # the radicand of alpha stays positive
            assert max(tr.thrust_area(f, s) for s in SPEEDS + [2.0])/((f.get('projected_diameter') or f['diameter'])*H.min()) < 1.0
    dt = 3.0
    out, lists = [], []
    for with_farms in (False, True):
        dev = _device(mesh, bath, dt)
        if visc:
            dev.set_viscosity(20.0 + 5.0*np.arange(mesh.num_vertices)/mesh.num_vertices)
        if with_farms:
            for i, f in enumerate(farms_c):
                dev.turbine_farm_set(i, _params(f), f['density'])
            for i, f in enumerate(farms_d):
                _set(dev, len(farms_c) + i, f, npc)
                lists.append(dev.dfarm_density_read(len(farms_c) + i)[0])
        dev.set_state(uv, eta)
        out.append(dev.tendency())
        dev.close()
    (ku0, ke0), (ku1, ke1) = out
    share = sum(dr.drag_tendency(orc, f, uv, eta, dt) for f in farms_d)
    if farms_c:
        share = share + tr.drag_tendency(orc, farms_c, uv, eta, dt)
    full = np.abs(ku1).max()
    err = np.abs((ku1 - ku0) - share).max()/full
    print('discrete farm share', kind, label, 'error / |full tendency|', err, ' share / full', np.abs(share).max()/full,
          'list lengths', [len(c) for c in lists])
    assert np.abs(share).max() > 1e-6*full                         # not vacuous
    assert err < TOL_RHS
    assert np.array_equal(ke0, ke1)
    if not farms_c:                                                # cells outside the lists: the bits of a handle without farms
        outside = np.ones(mesh.num_cells, dtype=bool)
        for c in lists:
            outside[c] = False
        assert np.array_equal(ku1[outside], ku0[outside]) and outside.any()
    return lists


def _continuous(mesh):
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    v = 2e-7*np.random.default_rng(101).uniform(0.2, 1.0, size=mesh.num_vertices)
    return dict(diameter=60.0, thrust=0.6, density=np.where(((xc > 30e3) & (xc < 60e3))[:, None], v[mesh.cells], 0.0))


@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
@pytest.mark.parametrize('config', ['constant', 'table_upwind_support', 'continuous_and_discrete', 'viscosity'])
def test_drag_share_of_the_tendency(hip_lib, kind, config):
    if config == 'constant':
        _share_check(kind, [_farm], label=config)
    elif config == 'table_upwind_support':
        _share_check(kind, [_table_farm], label=config)
    elif config == 'continuous_and_discrete':
        _share_check(kind, [_table_farm, lambda m: _farm(m, coords=COORDS[1:3], edge=1e9, projected_diameter=12e3)], [_continuous], label=config)
    else:
        _share_check(kind, [_table_farm], visc=True, label=config)


@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
@pytest.mark.parametrize('degree', [3, 14])
def test_drag_share_at_the_smallest_and_the_largest_rule(hip_lib, kind, degree):
    _share_check(kind, [lambda m: _table_farm(m, degree=degree)], label='degree {:d}'.format(degree))


# ---- 3. stepping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
def test_twenty_steps_against_the_oracle_with_the_reference_term(hip_lib, kind):
    mesh, bath, uv, eta, orc_of = _case(kind, seed=4)
    npc = mesh.cells.shape[1]
    farm = _table_farm(mesh)
    orc = orc_of(mesh, bath)
    plain = orc.tendency

    def with_farm(u, e, dt, time=0.0):
        ku, ke = plain(u, e, dt, time)
        return ku + dr.drag_tendency(orc, farm, u, e, dt), ke
    orc.tendency = with_farm
    dt = 3.0
    uv0, eta0 = 1.5*uv, eta                                        # most of the flow above the table's cut-in speed
    dev = _device(mesh, bath, dt)
    _set(dev, 0, farm, npc)
    for name, step, advance in (('SSPRK33', orc.ssprk33_step, dev.advance), ('ForwardEuler', orc.forward_euler_step, dev.advance_forward_euler)):
        dev.set_state(uv0, eta0)
        advance(20)
        ud, ed = dev.get_state()
        uo, eo = uv0, eta0
        for _ in range(20):
            uo, eo = step(uo, eo, dt)
        print('20 steps', name, kind, rel_linf(ud, uo), rel_linf(ed, eo))
        assert rel_linf(ud, uo) < 1e-11 and rel_linf(ed, eo) < 1e-11
    # the farm is felt: without it the run ends elsewhere
    twin = _device(mesh, bath, dt)
    twin.set_state(uv0, eta0)
    twin.advance_forward_euler(20)
    assert rel_linf(twin.get_state()[0], ud) > 1e-9
    twin.close()
    dev.close()


@pytest.mark.parametrize('quads', [False, True])
def test_every_path_setting_gives_the_bits_of_stage_launches(hip_lib, quads):
    from thetis_amd import _lib
    mesh, bath, uv, eta = quad_case(40, 16, amp_eta=0.1, amp_u=0.3) if quads else channel_case(40, 16, amp_eta=0.1, amp_u=0.3)
    bath = bath + 20.0
    npc = mesh.cells.shape[1]
    farm = _table_farm(mesh)
    res = []
    for fused in (None, 0, 1, 2, 3):
        for flow in (None, 0):
            for staged in ((True, False) if fused is None and flow is None else (False,)):
                dev = _device(mesh, bath, 2.0)
                if fused is not None:
                    dev.set_option(_lib.OPT_FUSED_STAGES, fused)
                if flow is not None:
                    dev.set_option(_lib.OPT_FLOW, flow)
                _set(dev, 1, farm, npc)
                assert dev.flow_supported() == 0
                assert not dev.fused_pair_info()[0] and not dev.fused_triple_info()[0] and not dev.fused_step_info()[0]
                dev.set_state(1.5*uv, eta)
                for _ in range(4):
                    if staged:
                        for i in range(3):
                            dev.solve_stage(i)
                    else:
                        dev.advance(1)
                res.append(dev.get_state())
                dev.turbine_farm_clear(1)
                assert quads or dev.flow_supported() in (1, 2)     # the slot is empty again: covered as before
                dev.close()
    assert all(np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) for r in res[1:])


@pytest.mark.parametrize('kind', ['tri', 'quad_general'])
def test_a_farm_with_an_empty_list_gives_the_bits_of_no_farm(hip_lib, kind):
    mesh, bath, uv, eta, orc_of = _case(kind, seed=6)
    npc = mesh.cells.shape[1]
    res = []
    for coords in (None, [], [COORDS[6]]):
        dev = _device(mesh, bath, 3.0)
        if coords is not None:
            _set(dev, 0, _table_farm(mesh, coords=coords), npc)
            assert len(dev.dfarm_density_read(0)[0]) == 0 and dev.flow_supported() == 0
            assert not dev.turbine_power().any() and len(dev.dfarm_turbine_power(0)) == len(coords)
            assert not dev.dfarm_turbine_power(0).any()
        dev.set_state(uv, eta)
        t = dev.tendency()
        dev.advance(3)
        dev.advance_forward_euler(2)
        res.append(t + dev.get_state())
        dev.close()
    for r in res[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, res[0]))


# ---- 4. the ends of the cell lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_list', [1, 256, 257])
def test_lists_of_one_and_around_four_waves(hip_lib, n_list):
    """One row of 300 quadrilaterals, 1 km wide: the square of one turbine covers exactly n_list of them (a structured triangle mesh
    lists its cells in pairs, both halves of a rectangle share the bounding box).  256 / 257: the last block of the pass full / one lane."""
    x_t, r = {1: (150500.0, 400.0), 256: (150000.0, 127900.0), 257: (150500.0, 128400.0)}[n_list]
    y_t = 30e3*0.5*(1.0 - 0.2386191860831969)                      # at a Gauss point of the 30 km high cells: the small square holds points

    def farm(mesh):
        return _farm(mesh, coords=[[x_t, y_t]], edge=1e9, diameter=400.0, projected_diameter=2*r, thrust=0.8)
    lists = _share_check('quad', [farm], mesh_kw=dict(nx=300, ny=1, lx=300e3, amp_u=0.3), label='n_list {:d}'.format(n_list))
    assert len(lists[0]) == n_list


# ---- 5. power -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
def test_power_per_farm_and_per_turbine(hip_lib, kind):
    mesh, bath, uv, eta, orc_of = _case(kind, seed=6)
    npc = mesh.cells.shape[1]
    uv = _scaled(uv, mesh, seed=8)
    orc = orc_of(mesh, bath)
    farms = [_farm(mesh), _table_farm(mesh, degree=14),
             dict(_table_farm(mesh, degree=3, coords=COORDS[1:4]), power_table=[0.0, 0.3, 0.45, 0.1, 0.0])]
    dev = _device(mesh, bath, 3.0)
    for i, f in enumerate(farms):
        _set(dev, 2*i, f, npc)                                     # slots 0, 2, 4
    dev.set_state(uv, eta)
    p = dev.turbine_power()
    dev.turbine_rows_reserve(2)
    dev.turbine_rows_append()
    dev.turbine_rows_append()
    rows = dev.turbine_rows_read()
    assert rows.shape == (2, len(p)) and np.array_equal(rows[0], p) and np.array_equal(rows[1], p)
    assert not p[1::2].any() and not p[5:].any()
    limbs = dev.turbine_power_limbs()
    for i, f in enumerate(farms):
        ref = dr.power(orc, f, uv)
        got = p[2*i]
        n_t = len(f['coordinates'])
        each = dev.dfarm_turbine_power(2*i)
        each_ref = np.array([dr.power(orc, f, uv, only=t) for t in range(n_t)])
        print('power', kind, i, got, ref, abs(got - ref)/ref, 'sum of turbines', each.sum(), 'difference in eps', abs(each.sum() - got)/got/EPS)
        assert ref > 0 and abs(got - ref) <= 1e-13*ref and dev.limbs_to_double(limbs[2*i]) == got
        assert each.shape == (n_t,) and np.abs(each - each_ref).max() <= 1e-13*each_ref.max()
        assert abs(float(np.sum(each)) - got) <= (n_t + 2)*EPS*got
        if n_t == len(COORDS):
            assert each[6] == 0.0 and (each[:5] > 0).all()         # the turbine outside the mesh; the overlapping ones split the power
    dev.close()


# ---- 6. the time loop -----------------------------------------------------------------------------------------------------------------
def _farm_solver(tmp_path, batched, tide=False, end_steps=18, n_export=6, dt=10.0):
    from thetis_amd import (Constant, DetectorsCallback, DiscreteTidalTurbineFarmOptions, Function, FunctionSpace, RectangleMesh,
                            TidalTurbineFarmOptions, solver2d, turbines as tb)
    from thetis_amd.rungekutta import SSPRK33
    lx, ly = 100e3, 30e3
    mesh = RectangleMesh(40, 12, lx, ly, cell_marker_fn=lambda x, y: np.where((x > 30e3) & (x < 70e3), 2, 0))
    calls = []
    orig = SSPRK33.advance_steps

    def counting(self, t, n, **kw):
        calls.append(n)
        return orig(self, t, n, **kw)
    SSPRK33.advance_steps = counting
    try:
        P1 = FunctionSpace(mesh, 'CG', 1)
        s = solver2d.FlowSolver2d(mesh, Function(P1).assign(30.0))
        o = s.options
        o.timestep = dt
        o.simulation_export_time = n_export*dt
        o.simulation_end_time = (end_steps - 0.5)*dt
        o.no_exports = True
        o.swe_timestepper_type = 'SSPRK33'
        o.swe_timestepper_options.use_automatic_timestep = False
        o.output_directory = str(tmp_path)
        o.quadratic_drag_coefficient = Constant(0.0025)
        elev = Constant(0.5)
        if tide:
            from thetis_amd import HarmonicTidalForcing, get_functionspace
            fs = get_functionspace(mesh, 'CG', 1)
            n = fs.node_count()
            elev = HarmonicTidalForcing(Function(fs, name='tidal_elev'), np.array([1.405189e-4, 1.454441e-4]),
                                        np.stack([np.full(n, 0.5), np.full(n, 0.2)]), np.stack([np.full(n, 0.3), np.full(n, 1.0)]))
        s.bnd_functions['shallow_water'] = {1: {'elev': elev}, 2: {'elev': Constant(-0.5)}}
        d = DiscreteTidalTurbineFarmOptions()
        d.turbine_type = 'table'
        d.turbine_options.diameter = 60.0
        d.turbine_options.projected_diameter = 12e3
        d.break_even_wattage = 1e3
        d.turbine_coordinates = [[40e3, 10e3], [46e3, 14e3], [60e3, 20e3]]
        c = TidalTurbineFarmOptions()
        c.turbine_density = Constant(1e-7)
        o.tidal_turbine_farms[2] = [c]
        o.discrete_tidal_turbine_farms[2] = [d]
        s.create_equations()
        cb = tb.TurbineFunctionalCallback(s, append_to_log=False)
        s.add_callback(cb, 'timestep')
        det = DetectorsCallback(s, [(45e3, 12e3), (80e3, 5e3)], ['elev_2d', 'uv_2d'], 'gauges', export_to_hdf5=False)
        s.add_callback(det, 'timestep')
        s.assign_initial_conditions(elev=lambda x, y: 0.5 - x/lx, uv=Constant((1.5, 0.0)))
        if batched:
            s.iterate()
        else:
            for _ in s.create_iterator():
                pass
        return s, cb, det, calls
    finally:
        SSPRK33.advance_steps = orig


@pytest.mark.parametrize('tide', [False, True])
def test_batched_iterate_equals_the_step_loop(hip_lib, tmp_path, tide):
    a, cb_a, det_a, calls_a = _farm_solver(tmp_path / 'a', True, tide=tide)
    assert calls_a == [6]*3                                        # one advance_steps per export interval, with the tide too
    b, cb_b, det_b, calls_b = _farm_solver(tmp_path / 'b', False, tide=tide)
    assert calls_b == []
    assert len(cb_a.history) == len(cb_b.history) == 18
    assert cb_a.integrated_power == cb_b.integrated_power and cb_a.average_profit == cb_b.average_profit
    assert all(np.array_equal(np.array(x[1:]), np.array(y[1:])) and x[0] == y[0] for x, y in zip(cb_a.history, cb_b.history))
    assert len(det_a.history) == len(det_b.history) > 0
    assert all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(det_a.history, det_b.history))
    assert np.array_equal(a.fields.uv_2d.dat.data_ro, b.fields.uv_2d.dat.data_ro)
    assert np.array_equal(a.fields.elev_2d.dat.data_ro, b.fields.elev_2d.dat.data_ro)
    assert min(cb_a.average_power) > 0 and 2.5 < cb_a.cost[1] < 3.5
    farm = a.tidal_farms[1]
    each = farm.turbine_powers()
    assert each.shape == (3,) and (each > 0).all() and abs(each.sum() - farm.power_output()) <= 5*EPS*farm.power_output()


def test_refused_on_a_wetting_drying_handle_and_inside_a_capture(hip_lib):
    import torch
    from thetis_amd import _lib
    mesh, bath, uv, eta, orc_of = _case('tri', seed=9)
    farm = _table_farm(mesh)
    dev = _device(mesh, bath, 3.0)
    dev.set_wetting_and_drying(0.5)
    with pytest.raises(_lib.Swe2dError) as err:
        _set(dev, 0, farm, 3)
    assert err.value.code == _lib.ERR_UNSUPPORTED
    dev.set_state(uv, np.abs(eta))
    dev.advance(2)                                                 # the handle still steps
    assert np.isfinite(dev.get_state()[0]).all()
    dev.close()
    # inside a capture the set call is refused; a captured advance of a handle with a discrete farm replays
    dev = _device(mesh, bath, 3.0)
    _set(dev, 0, farm, 3)
    dev.set_state(1.5*uv, eta)
    dev.advance(4)
    want = dev.get_state()
    s = torch.cuda.Stream()
    dev.set_stream(s.cuda_stream)
    dev.set_state(1.5*uv, eta)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        dev.advance(1)                                             # warm-up on the stream
        s.synchronize()
        dev.set_state(1.5*uv, eta)
        with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
            with pytest.raises(_lib.Swe2dError) as err:
                _set(dev, 1, farm, 3)
            assert err.value.code == _lib.ERR_UNSUPPORTED
            dev.advance(2)
        g.replay()
        g.replay()
    s.synchronize()
    got = dev.get_state()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    dev.set_stream(None)
    dev.close()


# ---- 7. lifecycle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['tri', 'quad'])
def test_set_clear_set_again_destroy(hip_lib, kind):
    mesh, bath, uv, eta, orc_of = _case(kind, seed=10)
    npc = mesh.cells.shape[1]
    orc = orc_of(mesh, bath)
    first, second = _table_farm(mesh), _farm(mesh, coords=COORDS[:2], degree=14)
    dev = _device(mesh, bath, 3.0)
    dev.set_state(uv, eta)
    _set(dev, 3, first, npc)
    assert len(dev.dfarm_turbine_power(3)) == len(COORDS) and dev.turbine_power()[3] > 0
    dev.turbine_farm_clear(3)
    assert not dev.turbine_power().any()
    dev.turbine_farm_clear(3)                                      # an empty slot: nothing to do
    _set(dev, 3, second, npc)
    _set(dev, 3, second, npc)                                      # ... and a replacement in place
    ku1, _ = dev.tendency()
    p = dev.turbine_power()[3]
    each = dev.dfarm_turbine_power(3)
    dev.turbine_farm_clear(3)
    ku0, _ = dev.tendency()
    share = dr.drag_tendency(orc, second, uv, eta, 3.0)
    assert np.abs((ku1 - ku0) - share).max() < TOL_RHS*np.abs(ku1).max() and np.abs(share).max() > 1e-6*np.abs(ku1).max()
    ref = dr.power(orc, second, uv)
    assert abs(p - ref) <= 1e-13*ref and each.shape == (2,)
    # a continuous farm takes a slot a discrete one held, and the other way round
    dens = np.where((mesh.cell_xy()[:, :, 0].mean(axis=1) < 50e3)[:, None], 1e-7, 0.0)*np.ones((mesh.num_cells, npc))
    _set(dev, 0, second, npc)
    dev.turbine_farm_set(0, _params(second), dens)
    assert dev.turbine_power()[0] > 0
    _set(dev, 0, second, npc)
    assert abs(dev.turbine_power()[0] - ref) <= 1e-13*ref
    dev.close()


# ---- 8. the example -----------------------------------------------------------------------------------------------------------------
def test_discrete_turbines_example(hip_lib):
    r = subprocess.run([sys.executable, os.path.join('examples', 'discrete_turbines.py'), '--nx', '30', '--ny', '10', '--t-end', '300'],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    farms = [l.split() for l in lines if l.startswith('farm ')]
    turbines = [l.split() for l in lines if l.startswith('  turbine ')]
    assert len(farms) == 2 and len(turbines) == 9
    for f in farms:
        energy, total = float(f[f.index('energy') + 1]), float(f[f.index('turbines') + 1])
        assert energy > 0 and abs(energy - total) <= 1e-10*energy
