"""
Discrete tidal turbine farms, host side: the farm's quadrature rule (exactness, weights, point cap), the bump density and
``number_of_turbines`` of ``DiscreteTidalTurbineFarm`` against tests/discrete_turbine_ref.py, and what ``build_farms`` and the
steppers' farm upload accept and refuse.  No GPU.
"""
from math import factorial
from types import SimpleNamespace

import numpy as np
import pytest

import discrete_turbine_ref as dr
from helpers import channel_case, make_oracle, make_oracle_generic, quad_case

EPS = np.finfo(np.float64).eps


# ---- the rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npc', [3, 4])
@pytest.mark.parametrize('degree', [3, 10, 14])
def test_rule_is_exact_to_its_degree(npc, degree):
    from thetis_amd.function import farm_quadrature
    phi, w = farm_quadrature(npc, degree)
    assert phi.shape == (len(w), npc) and len(w) <= 64
    assert (w > 0).all() and abs(w.sum() - 1.0) <= 4*EPS
    assert np.abs(phi.sum(axis=1) - 1.0).max() <= 4*EPS
    # reference coordinates of the points from the basis values
    x, y = (phi[:, 1], phi[:, 2]) if npc == 3 else (phi[:, 1] + phi[:, 2], phi[:, 2] + phi[:, 3])
    area = 0.5 if npc == 3 else 1.0
    worst = 0.0
    for a in range(degree + 1):
        for b in range(degree + 1 - a):
            exact = factorial(a)*factorial(b)/factorial(a + b + 2) if npc == 3 else 1.0/((a + 1)*(b + 1))
            got = area*float(np.sum(w*x**a*y**b))
            worst = max(worst, abs(got - exact)/exact)
    print('rule', npc, degree, len(w), 'points, worst relative error', worst)
    assert worst <= 1e-14
    # ... and the package's rule is the reference statement's
    phi_r, w_r = dr.rule(npc, degree)
    assert np.abs(phi - phi_r).max() <= 2*EPS and np.abs(w - w_r).max() <= 2*EPS


def test_point_counts_and_cap():
    from thetis_amd import _lib
    from thetis_amd.function import MAX_FARM_QUAD, farm_quadrature
    assert MAX_FARM_QUAD == _lib.MAX_FARM_QUAD == 64
    assert [len(farm_quadrature(4, d)[1]) for d in (3, 10, 14)] == [4, 36, 64]
    assert [len(farm_quadrature(3, d)[1]) for d in (3, 10, 14)] == [6, 36, 64]
    with pytest.raises(NotImplementedError, match='quadrature_degree'):
        farm_quadrature(4, 16)
    with pytest.raises(NotImplementedError, match='quadrature_degree'):
        farm_quadrature(3, 15)


# ---- DiscreteTidalTurbineFarm ------------------------------------------------------------------------------------------------
def _farm(mesh, coordinates, diameter=9e3, subdomain='everywhere', degree=10, **turbine_kw):
    from thetis_amd.options import DiscreteTidalTurbineFarmOptions
    from thetis_amd.turbines import DiscreteTidalTurbineFarm
    o = DiscreteTidalTurbineFarmOptions()
    o.turbine_options.diameter = diameter
    o.quadrature_degree = degree
    o.turbine_coordinates = coordinates
    for k, v in turbine_kw.items():
        setattr(o.turbine_options, k, v)
    return DiscreteTidalTurbineFarm(mesh, subdomain, o)


def test_density_against_the_reference_statement():
    from thetis_amd import Constant
    mesh = channel_case(24, 8)[0]
    coords = [[40e3, 15e3], [43e3, 16e3], [Constant(80e3), Constant(5e3)]]
    farm = _farm(mesh, coords[:2])
    farm.add_turbines(coords[2:])
    assert farm.coordinates.shape == (3, 2) and farm.radius == 4.5e3 and farm.turbine_density == farm.density
    ref = dict(diameter=9e3, coordinates=[[40e3, 15e3], [43e3, 16e3], [80e3, 5e3]])
    rng = np.random.default_rng(0)
    xy = np.concatenate([rng.uniform([30e3, 8e3], [50e3, 22e3], size=(4000, 2)), rng.uniform([0, 0], [100e3, 30e3], size=(1000, 2))])
    peak = 2.0/(4.5e3**2*dr.BUMP_NORM)                              # two bumps overlap
    got, want = farm.density(xy), dr.density(ref, xy)
    print('density: max difference / peak', np.abs(got - want).max()/peak, 'max / peak', got.max()/peak)
    assert np.abs(got - want).max() <= 4*EPS*peak and got.max() > 0.5*peak
    # zero at and beyond |dx| = r, in either direction
    r = 4.5e3
    edge = np.array([[80e3 + r, 5e3], [80e3 - r, 5e3], [80e3, 5e3 + r], [80e3 + 1.5*r, 5e3], [80e3 + r, 5e3 + r]])
    assert not farm.density(edge).any()
    assert farm.density(np.array([[80e3 + r*(1 - 1e-9), 5e3]]))[0] >= 0.0
    # two overlapping turbines add
    one = _farm(mesh, coords[:1]).density(xy) + _farm(mesh, coords[1:2]).density(xy)
    both = _farm(mesh, coords[:2]).density(xy)
    assert np.array_equal(one, both) and ((_farm(mesh, coords[:1]).density(xy) > 0) & (_farm(mesh, coords[1:2]).density(xy) > 0)).any()


@pytest.mark.parametrize('kind', ['tri', 'quad', 'quad_general'])
def test_number_of_turbines_against_the_reference_statement(kind):
    if kind == 'tri':
        mesh, bath = channel_case(24, 8)[:2]
        orc = make_oracle(mesh, bath)
    else:
        mesh, bath = quad_case(24, 8, warp=0.2 if kind == 'quad_general' else 0.0)[:2]
        orc = make_oracle_generic(mesh, bath)
    coords = [[40e3, 15e3], [43e3, 16e3], [99e3, 5e3], [150e3, 5e3]]
    farm = _farm(mesh, coords)
    ref = dict(diameter=9e3, coordinates=coords, cells=np.ones(mesh.num_cells, dtype=bool), degree=10)
    got, want = farm.number_of_turbines(), dr.number_of_turbines(orc, ref)
    print('number_of_turbines', kind, got, want)
    assert abs(got - want) <= 1e-13*want and 2.0 < got < 3.0       # two whole bumps, one cut by the boundary, one outside


def test_number_of_turbines_accuracy_figure():
    """An accuracy figure, no assertion on it: one interior turbine, cells of size r, r/2, r/4.  The integrand is
    not a polynomial and the norm 1.45661 has five digits."""
    r = 2e3
    for n in (1, 2, 4):
        from thetis_amd import RectangleMesh
        for quad in (False, True):
            mesh = RectangleMesh(10*n, 6*n, 10*r, 6*r, quadrilateral=quad)
            farm = _farm(mesh, [[4.3*r, 3.1*r]], diameter=2*r)
            print('number_of_turbines, cell size r/{:d}, {:s}: {:.9f}'.format(n, 'quadrilaterals' if quad else 'triangles', farm.number_of_turbines()))
            assert np.isfinite(farm.number_of_turbines())


# ---- build_farms and the upload ------------------------------------------------------------------------------------------------
def _solver(mesh):
    from thetis_amd import Function, get_functionspace, solver2d
    s = solver2d.FlowSolver2d(mesh, Function(get_functionspace(mesh, 'CG', 1)).assign(30.0))
    s.options.swe_timestepper_type = 'SSPRK33'
    return s


def _marked_mesh():
    from thetis_amd import RectangleMesh
    return RectangleMesh(8, 4, 80e3, 40e3, cell_marker_fn=lambda x, y: np.where((x > 30e3) & (x < 50e3), 2, 0))


def test_build_farms_with_a_discrete_farm_no_longer_raises():
    """the test that fails without the feature: the old message is gone, the farm is built"""
    from thetis_amd.options import DiscreteTidalTurbineFarmOptions
    from thetis_amd.turbines import DiscreteTidalTurbineFarm
    s = _solver(_marked_mesh())
    d = DiscreteTidalTurbineFarmOptions()
    d.turbine_coordinates = [[40e3, 20e3], [45e3, 10e3]]
    s.options.discrete_tidal_turbine_farms[2] = [d]
    s.create_equations()
    assert len(s.tidal_farms) == 1 and isinstance(s.tidal_farms[0], DiscreteTidalTurbineFarm)
    f = s.tidal_farms[0]
    assert f.coordinates.shape == (2, 2) and f.cells.sum() == 16 and f.quadrature_degree == 10 and f.turbine.upwind_correction
    assert f._solver is s and f._index == 0
    assert float(f.friction_coefficient(np.array([1.0, 0.0]), 40.0)) == pytest.approx(float(f.turbine.friction_coefficient(np.array([1.0, 0.0]), 40.0)))


def test_build_farms_order_type_error_and_limits():
    from thetis_amd import Constant
    from thetis_amd.options import DiscreteTidalTurbineFarmOptions, TidalTurbineFarmOptions
    from thetis_amd.turbines import DiscreteTidalTurbineFarm, TidalTurbineFarm
    mesh = _marked_mesh()
    c = TidalTurbineFarmOptions()
    c.turbine_density = Constant(1e-5)
    d = DiscreteTidalTurbineFarmOptions()
    d.turbine_coordinates = [[40e3, 20e3]]
    # continuous farms first, then discrete ones, each in the order of its dict
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms['everywhere'] = [d, d]
    s.options.tidal_turbine_farms[2] = [c]
    s.create_equations()
    kinds = [type(f) for f in s.tidal_farms]
    assert kinds == [TidalTurbineFarm, DiscreteTidalTurbineFarm, DiscreteTidalTurbineFarm]
    assert [f._index for f in s.tidal_farms] == [0, 1, 2] and s.tidal_farms[1].cells.all()
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[2] = d                 # not a list
    with pytest.raises(TypeError):
        s.create_equations()
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[7] = [d]               # no such subdomain
    with pytest.raises(ValueError):
        s.create_equations()
    # stated limits
    g = DiscreteTidalTurbineFarmOptions()
    g.turbine_options.apply_shear_profile = True
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[2] = [g]
    with pytest.raises(NotImplementedError, match='apply_shear_profile'):
        s.create_equations()
    s = _solver(mesh)
    s.options.tidal_turbine_farms[2] = [c]*5
    s.options.discrete_tidal_turbine_farms[2] = [d]*4
    with pytest.raises(NotImplementedError, match='SWE2D_MAX_FARMS'):
        s.create_equations()
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[2] = [d, DiscreteTidalTurbineFarmOptions()]      # the second has no turbines
    with pytest.raises(NotImplementedError, match='turbine_coordinates'):
        s.create_equations()
    q = DiscreteTidalTurbineFarmOptions()
    q.quadrature_degree = 16
    s = _solver(mesh)
    s.options.discrete_tidal_turbine_farms[2] = [q]
    with pytest.raises(NotImplementedError, match='quadrature_degree'):
        s.create_equations()
    s = _solver(mesh)
    s.options.use_wetting_and_drying = True
    s.options.discrete_tidal_turbine_farms[2] = [d]
    with pytest.raises(NotImplementedError, match='use_wetting_and_drying'):
        s.create_equations()


def test_upload_refuses_several_ranks_and_a_device_without_discrete_farms():
    from cpu_device import CpuSwe2dDevice
    from thetis_amd.rungekutta import SSPRK33
    farm = _farm(_marked_mesh(), [[40e3, 20e3]])
    stepper = object.__new__(SSPRK33)
    stepper.equation = SimpleNamespace(tidal_farms=[farm])
    stepper._farm_signatures = {}
    stepper.comm = SimpleNamespace(size=2)
    with pytest.raises(NotImplementedError, match='several ranks'):
        stepper._push_farms()
    stepper.comm = SimpleNamespace(size=1)
    assert not hasattr(CpuSwe2dDevice, 'dfarm_set')
    stepper.device = object.__new__(CpuSwe2dDevice)               # the host stand-in
    with pytest.raises(NotImplementedError, match='discrete_tidal_turbine_farms'):
        stepper._push_farms()
    # a device with the call takes the farm once, and again after turbines were added
    calls = []
    stepper.device = SimpleNamespace(dfarm_set=lambda *a: calls.append(a), turbine_farm_set=None)
    stepper._push_farms()
    stepper._push_farms()
    assert len(calls) == 1 and calls[0][0] == 0 and calls[0][2].shape == (1, 2) and calls[0][3].all() and calls[0][4].shape == (36, 3)
    farm.add_turbines([[45e3, 10e3]])
    stepper._push_farms()
    assert len(calls) == 2 and calls[1][2].shape == (2, 2)
