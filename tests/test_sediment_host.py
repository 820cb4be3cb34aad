"""The sediment stepper's host fallback through FlowSolver2d (``-m "not gpu"``): a device class without the sediment calls gets the
source per stage, the 'equilibrium' values and the Exner update from ``HostSediment``.  The stand-in device is tests/cpu_device.py's
with the three calls the fallback needs; its tracer boundaries take constants, which is all a uniform flow asks for."""
import numpy as np
import pytest

from cpu_device import CpuSwe2dDevice
from sediment_cases import D50, KS, NU
from thetis_amd import options as o
from thetis_amd.function import Function, get_functionspace
from thetis_amd.mesh import RectangleMesh
from thetis_amd.solver2d import FlowSolver2d

DEPTH, SPEED, DT = 0.397, 0.5, 0.2


class HostSedimentDevice(CpuSwe2dDevice):
    """no sediment_set / sediment_update / exner_step: the stepper takes the host path"""

    def tracer_get_buffer(self, tid, i_buffer):
        return self.tracers[tid]['T'][int(i_buffer)].copy()

    def tracer_set_bc_facets(self, tid, slot, values):
        v = np.asarray(values, dtype=np.float64)
        assert np.ptp(v) == 0.0, 'the stand-in takes constant boundary values only'
        self.tracers[tid]['bc'][int(slot)] = float(v.flat[0])
        self.tracers[tid]['rt'] = None

    def set_bathymetry(self, vertex_values):
        self.h = np.asarray(vertex_values, dtype=np.float64)[self.cells]
        self._dirty()


def _solver(solve_exner=False, morfac=1.0, device_cls=HostSedimentDevice):
    mesh = RectangleMesh(4, 3, 16.0, 1.1)
    bath = Function(get_functionspace(mesh, 'CG', 1), name='bathymetry_2d').assign(DEPTH)
    s = FlowSolver2d(mesh, bath)
    s._device_cls = device_cls
    m, so = s.options, s.options.sediment_model_options
    so.solve_suspended_sediment = True
    so.solve_exner = solve_exner
    so.use_advective_velocity_correction = False
    so.average_sediment_size = o.Constant(D50)
    so.bed_reference_height = o.Constant(KS)
    so.morphological_acceleration_factor = o.Constant(morfac)
    m.horizontal_viscosity = None
    so.morphological_viscosity = o.Constant(NU)
    m.tracer_only = True
    m.no_exports = True
    m.set_timestepper_type('SSPRK33')
    if solve_exner:
        so.exner_timestepper_type = 'ForwardEuler'
    for t in (m.swe_timestepper_options, m.tracer_timestepper_options, so.sediment_timestepper_options):
        t.use_automatic_timestep = False
    m.timestep = DT
    m.simulation_export_time = 100*DT
    uv = Function(get_functionspace(mesh, 'DG', 1, vector=True))
    uv.dat.data[:, 0] = SPEED
    return s, uv


def test_relaxation_closed_form_on_the_host_path():
    """tracer_only, uniform uv and depth on the closed 4 x 3 mesh, S0 = 0, SSPRK33: every node follows
    S_{n+1} = S_eq + (S_n - S_eq) P(z), z = -D dt/H, P = 1 + z + z^2/2 + z^3/6, for 10 steps, to 1e-13 of S_eq"""
    s, uv = _solver()
    s.options.simulation_end_time = 10*DT
    s.assign_initial_conditions(uv=uv, sediment=o.Constant(0.0))
    ts = s.timestepper.tracers['sediment_2d']
    assert ts.host_sediment and not s.sediment_model.on_device
    D, eq = s.sediment_model.get_deposition_coefficient(), s.sediment_model.get_equilibrium_tracer()
    assert np.ptp(D) == 0 and np.ptp(eq) == 0 and eq[0, 0] > 0
    s_eq, z = float(eq[0, 0]), -float(D[0, 0])*DT/DEPTH
    P = 1 + z + z*z/2 + z**3/6
    S, worst, n = 0.0, 0.0, 0
    for _ in s.create_iterator():
        S = s_eq + (S - s_eq)*P
        worst = max(worst, float(np.abs(s.fields.sediment_2d.dat.data_ro - S).max())/s_eq)
        n += 1
    print('relaxation on the host path: largest deviation {:.3e} of S_eq'.format(worst))
    assert n == 10 and worst <= 1e-13


def test_equilibrium_is_a_fixed_point_on_the_host_path():
    """S = S_eq everywhere, uniform flow through the channel, 'equilibrium' at the inflow and an open outflow, tracer_only,
    solve_exner, 5 steps: S stays within 1e-13 relative, the bed moves by at most 5 dt fac E 1e-12"""
    s, uv = _solver(solve_exner=True, morfac=100.0)
    s.options.simulation_end_time = 5*DT
    s.bnd_functions['sediment'] = {1: {'equilibrium': None}, 2: {}}
    s.assign_initial_conditions(uv=uv)                      # no initial field: the sediment starts at its equilibrium
    model = s.sediment_model
    E, eq = model.get_erosion_term(), model.get_equilibrium_tracer().copy()
    assert np.array_equal(s.fields.sediment_2d.dat.data_ro.reshape(eq.shape), eq) and eq.min() > 0
    bed0 = s.fields.bathymetry_2d.dat.data_ro.copy()
    s.iterate()
    assert s.iteration == 5
    drift = float(np.abs(s.fields.sediment_2d.dat.data_ro.reshape(eq.shape) - eq).max()/eq.max())
    moved = float(np.abs(s.fields.bathymetry_2d.dat.data_ro - bed0).max())
    bound = 5*DT*model.constants['fac']*float(E.max())*1e-12
    print('fixed point on the host path: drift {:.3e}, bed moved {:.3e} (bound {:.3e})'.format(drift, moved, bound))
    assert drift <= 1e-13 and moved <= bound


def test_a_device_without_the_calls_the_fallback_needs_is_refused():
    s, uv = _solver(device_cls=CpuSwe2dDevice)
    with pytest.raises(NotImplementedError, match='tracer_get_buffer'):
        s.assign_initial_conditions(uv=uv)
