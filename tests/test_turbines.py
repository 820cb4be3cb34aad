"""
Tidal turbine farms, host side: the numpy statement of the terms (tests/turbine_ref.py) pinned against hand values, the options
with the reference's names and defaults, the stated limits, and cell subdomain ids through the mesh classes, the partitioner and
MSH files.  No GPU.
"""
import numpy as np
import pytest

import turbine_ref as tr
from helpers import channel_case, make_oracle, make_oracle_generic, quad_case


SPEEDS = [0.9, 1., 3., 5., 5.001]
C_T = [0.01, 0.7, 0.7, 0.1, 0.0001]


# ---- the reference statement against hand values ---------------------------------------------------------------------------
def test_table_at_between_below_and_beyond_the_entries():
    s = np.array([0.0, 0.5, 0.8999, 0.9, 0.95, 1.0, 2.0, 3.0, 4.0, 5.0, 5.0005, 5.001, 5.5, 100.0])
    expect = np.interp(s, SPEEDS, C_T)
    expect[s < SPEEDS[0]] = 0.0
    expect[s >= SPEEDS[-1]] = 0.0
    assert np.array_equal(tr.table(SPEEDS, C_T, s), expect)
    assert tr.table(SPEEDS, C_T, 0.9) == 0.01 and tr.table(SPEEDS, C_T, 5.001) == 0.0 and tr.table(SPEEDS, C_T, 0.95) == pytest.approx(0.355)
    # the package's own table agrees
    from thetis_amd.turbines import TabulatedThrustTurbine
    from thetis_amd.options import TabulatedTidalTurbineOptions
    t = TabulatedThrustTurbine(TabulatedTidalTurbineOptions())
    got = t.thrust_coefficient(np.stack([s, 0*s], axis=1))
    assert np.allclose(got, expect, rtol=1e-15, atol=0)


def test_power_coefficient_default_and_alpha_worked_value():
    assert tr.default_power_coefficient(0.8) == 0.5*0.8*(1 + np.sqrt(0.2))
    farm = dict(diameter=20.0, projected_diameter=25.0, thrust=0.64, C_support=0.5, A_support=10.0, upwind=True)
    fric = 0.64*np.pi*100.0 + 5.0
    a = 0.5*(1 + np.sqrt(1 - fric/(25.0*40.0)))
    assert tr.thrust_area(farm, 1.0) == pytest.approx(fric, rel=1e-15)
    assert float(tr.alpha(farm, 1.0, 40.0)) == pytest.approx(a, rel=1e-15)
    assert float(tr.c_t(farm, 1.0, 40.0)) == pytest.approx(fric/2/a**2, rel=1e-15)
    from thetis_amd.turbines import ConstantThrustTurbine
    from thetis_amd.options import ConstantTidalTurbineOptions
    o = ConstantTidalTurbineOptions()
    o.diameter, o.projected_diameter, o.thrust_coefficient, o.C_support, o.A_support = 20.0, 25.0, 0.64, 0.5, 10.0
    t = ConstantThrustTurbine(o, upwind_correction=True)
    assert float(t.friction_coefficient(np.array([1.0, 0.0]), 40.0)) == pytest.approx(fric/2/a**2, rel=1e-14)
    assert t.C_P == 0.5*0.64*(1 + (1 - 0.64)**0.5)


def _band(mesh, lo, hi):
    xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
    return (xc > lo) & (xc < hi)


@pytest.mark.parametrize('quads', [False, True])
def test_uniform_flow_over_a_flat_farm_closed_forms(quads):
    if quads:
        mesh, bath, uv, eta = quad_case()
        bath = np.full(mesh.num_vertices, 30.0)
        orc = make_oracle_generic(mesh, bath)
    else:
        mesh, bath, uv, eta = channel_case(flat=True)
        bath = np.full(mesh.num_vertices, 30.0)
        orc = make_oracle(mesh, bath)
    k = mesh.cells.shape[1]
    inside = _band(mesh, 30e3, 70e3)
    assert inside.any() and not inside.all()
    dens = 2.5e-5
    farm = dict(diameter=18.0, thrust=0.8, density=np.where(inside[:, None], dens, 0.0)*np.ones((mesh.num_cells, k)))
    area = float(mesh.cell_areas()[inside].sum())
    assert tr.number_of_turbines(orc, farm) == pytest.approx(dens*area, rel=1e-14)
    u0 = np.array([1.2, -0.5])
    uv = np.broadcast_to(u0, (mesh.num_cells, k, 2)).copy()
    eta = np.zeros((mesh.num_cells, k))
    speed = float(np.hypot(*u0))
    a_t = np.pi*18.0**2/4
    p_exact = 0.5*1000.0*a_t*tr.default_power_coefficient(0.8)*speed**3*dens*area
    assert tr.power(orc, farm, uv) == pytest.approx(p_exact, rel=1e-14)
    # the term: M^-1 dt F with constant integrand = -dt c_t d |u| u / H at every node of a farm cell, zero elsewhere
    dt = 7.0
    ku = tr.drag_tendency(orc, [farm], uv, eta, dt)
    exact = -dt*(0.8*a_t/2)*dens*speed*u0/30.0
    assert np.abs(ku[inside] - exact).max() <= 1e-14*np.abs(exact).max()*4
    assert not ku[~inside].any()


# ---- options -------------------------------------------------------------------------------------------------------------
def test_option_defaults_and_validation():
    from thetis_amd.options import (ConstantTidalTurbineOptions, ModelOptions2d, TabulatedTidalTurbineOptions, TidalTurbineFarmOptions,
                                    TidalTurbineOptions)
    t = TidalTurbineOptions()
    assert (t.diameter, t.projected_diameter, t.C_support, t.A_support, t.apply_shear_profile) == (18.0, None, 0.0, 0.0, False)
    c = ConstantTidalTurbineOptions()
    assert c.thrust_coefficient == 0.8 and c.power_coefficient is None
    tab = TabulatedTidalTurbineOptions()
    assert tab.thrust_speeds == SPEEDS and tab.thrust_coefficients == C_T and tab.power_coefficients is None
    f = TidalTurbineFarmOptions()
    assert f.turbine_type == 'constant' and isinstance(f.turbine_options, ConstantTidalTurbineOptions)
    assert float(f.turbine_density) == 0.0 and f.break_even_wattage == 0.0 and getattr(f, 'upwind_correction', False) is False
    f.turbine_type = 'table'
    assert isinstance(f.turbine_options, TabulatedTidalTurbineOptions)
    with pytest.raises(ValueError):
        f.turbine_type = 'bladeless'
    with pytest.raises(TypeError):
        f.no_such_option = 1
    with pytest.raises(AssertionError):
        c.diameter = -1.0
    o = ModelOptions2d()
    assert o.tidal_turbine_farms == {} and o.discrete_tidal_turbine_farms == {}


def _solver(mesh, **farm_kw):
    from thetis_amd import Function, get_functionspace, solver2d
    bath = Function(get_functionspace(mesh, 'CG', 1)).assign(30.0)
    s = solver2d.FlowSolver2d(mesh, bath)
    s.options.swe_timestepper_type = 'SSPRK33'
    return s


def test_farm_list_type_error_subdomain_and_limits():
    from thetis_amd import Constant, RectangleMesh
    from thetis_amd.options import DiscreteTidalTurbineFarmOptions, TidalTurbineFarmOptions
    mesh = RectangleMesh(8, 4, 80e3, 40e3, cell_marker_fn=lambda x, y: np.where((x > 30e3) & (x < 50e3), 2, 0))
    f = TidalTurbineFarmOptions()
    f.turbine_density = Constant(1e-5)
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = f                          # not a list
    with pytest.raises(TypeError):
        s.create_equations()
    s = _solver(mesh)
    s.options.tidal_turbine_farms[7] = [f]                        # no such subdomain
    with pytest.raises(ValueError):
        s.create_equations()
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [f, f]
    s.options.tidal_turbine_farms['everywhere'] = [f]
    s.create_equations()
    assert len(s.tidal_farms) == 3 and 'TurbineDragTerm' in s.equations.sw.SUPPORTED_TERMS
    assert s.tidal_farms[0].cells.sum() == 16 and s.tidal_farms[2].cells.all()
    assert s.tidal_farms[0].number_of_turbines() == pytest.approx(1e-5*20e3*40e3, rel=1e-14)
    assert s.tidal_farms[0].break_even_wattage == 0.0 and s.tidal_farms[0].turbine.C_T == 0.8
    s = _solver(mesh)
    s.create_equations()
    assert s.tidal_farms is None
    # stated limits
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[2] = [DiscreteTidalTurbineFarmOptions()]
    with pytest.raises(NotImplementedError, match='discrete_tidal_turbine_farms'):
        s.create_equations()
    g = TidalTurbineFarmOptions()
    g.turbine_options.apply_shear_profile = True
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [g]
    with pytest.raises(NotImplementedError, match='apply_shear_profile'):
        s.create_equations()
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [f]*9
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_FARMS'):
        s.create_equations()
    t = TidalTurbineFarmOptions()
    t.turbine_type = 'table'
    t.turbine_options.thrust_speeds = list(np.linspace(0.5, 5.0, 17))
    t.turbine_options.thrust_coefficients = [0.5]*17
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [t]
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_THRUST_TABLE'):
        s.create_equations()
    t.turbine_options.thrust_coefficients = [0.5]*16              # lengths differ
    with pytest.raises(ValueError):
        s.create_equations()


def test_density_is_zeroed_outside_the_farm():
    from thetis_amd import Function, RectangleMesh, get_functionspace
    from thetis_amd.options import TidalTurbineFarmOptions
    mesh = RectangleMesh(8, 4, 80e3, 40e3, cell_marker_fn=lambda x, y: np.where((x > 30e3) & (x < 50e3), 2, 0))
    d = Function(get_functionspace(mesh, 'CG', 1)).interpolate(lambda x, y: 1e-5*(1 + x/80e3))
    f = TidalTurbineFarmOptions()
    f.turbine_density = d
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [f]
    s.create_equations()
    farm = s.tidal_farms[0]
    nodal = farm.density_nodal()
    assert nodal.shape == (mesh.num_cells, 3) and not nodal[mesh.cell_markers != 2].any() and (nodal[mesh.cell_markers == 2] > 0).all()
    assert np.array_equal(nodal[mesh.cell_markers == 2], d.dat.data_ro[mesh.cells][mesh.cell_markers == 2])
    sig = farm.density_signature()
    d.assign(2e-5)
    assert farm.density_signature() != sig


# ---- cell subdomain ids ----------------------------------------------------------------------------------------------------
def test_cell_markers_default_renumbered_partition_and_msh(tmp_path):
    from thetis_amd import RectangleMesh, read_gmsh, write_gmsh
    from thetis_amd.partition import build_partition, strip_owner
    plain = RectangleMesh(6, 4, 6.0, 4.0)
    assert plain.cell_markers.dtype == np.int32 and not plain.cell_markers.any()
    for quad in (False, True):
        mesh = RectangleMesh(6, 4, 6.0, 4.0, quadrilateral=quad, cell_marker_fn=lambda x, y: np.where(x > 3.0, 5, np.where(y > 2.0, 3, 0)))
        xc = mesh.cell_xy().mean(axis=1)
        expect = np.where(xc[:, 0] > 3.0, 5, np.where(xc[:, 1] > 2.0, 3, 0))
        assert np.array_equal(mesh.cell_markers, expect) and set(expect) == {0, 3, 5}
        perm = np.random.default_rng(3).permutation(mesh.num_cells)
        assert np.array_equal(mesh.renumbered(perm).cell_markers, expect[perm])
        owner = strip_owner(mesh, 3)
        for r in range(3):
            part = build_partition(mesh, owner, r, halo_depth=1)
            assert np.array_equal(part.cell_markers, expect[part.local_to_global])
        path = str(tmp_path / ('q.msh' if quad else 't.msh'))
        write_gmsh(mesh, path)
        back = read_gmsh(path)
        assert np.array_equal(back.cell_markers, expect)
        assert np.array_equal(back.cell_nbr, mesh.cell_nbr)
    # a file whose cells carry no tags reads as before, markers 0
    path = str(tmp_path / 'untagged.msh')
    write_gmsh(plain, path)
    text = open(path).read().replace(' 2 2 1 1 ', ' 2 0 ')
    open(path, 'w').write(text)
    back = read_gmsh(path)
    assert not back.cell_markers.any() and np.array_equal(back.cells, plain.cells)


def test_farms_on_several_ranks_raise():
    """the partitioned driver does not carry farms: uploading them with a communicator of more than one rank names the option"""
    from types import SimpleNamespace
    from thetis_amd.rungekutta import SSPRK33
    stepper = object.__new__(SSPRK33)
    stepper.equation = SimpleNamespace(tidal_farms=[object()])
    stepper.comm = SimpleNamespace(size=2)
    stepper._farm_signatures = {}
    with pytest.raises(NotImplementedError, match='tidal_turbine_farms'):
        stepper._push_farms()
    stepper.comm = SimpleNamespace(size=1)
    stepper.device = object()                                     # a device class without the farm calls
    with pytest.raises(NotImplementedError, match='tidal_turbine_farms'):
        stepper._push_farms()
    stepper.equation = SimpleNamespace(tidal_farms=None)
    stepper._push_farms()                                         # nothing to upload: no device call, no raise
