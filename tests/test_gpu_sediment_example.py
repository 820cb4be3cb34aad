"""examples/sediment_trench.py through FlowSolver2d on the device: it runs, the bed moves with the signs the set-up implies at two
named vertices, the sediment-mass callback prints; iterate()'s batches equal the step-by-step loop bit for bit for both sediment
steppers."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location('sediment_trench', os.path.join(ROOT, 'examples', 'sediment_trench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trench_example(capsys):
    """The sediment starts at its local equilibrium, which is lower inside the trench (slower flow) than outside.  Advection and the
    sediment diffusivity carry sediment from the approach into the trench: at the trench's upstream edge the concentration falls
    below the local equilibrium - the bed erodes (the bathymetry, positive downwards, grows); where the floor begins behind the
    upstream slope it rises above it - the bed accretes."""
    mod = _example()
    solver = mod.main(['--nx', '32', '--ny', '2', '--steps', '48'])
    out = capsys.readouterr().out
    assert 'sediment_2d mass' in out and 'bed change' in out
    xy = solver.mesh2d.vertex_xy
    edge = int(np.argmin(np.abs(xy[:, 0] - 5.0) + np.abs(xy[:, 1])))      # vertex (5.0, 0): the trench's upstream edge
    floor = int(np.argmin(np.abs(xy[:, 0] - 6.5) + np.abs(xy[:, 1])))     # vertex (6.5, 0): where the floor begins
    assert np.allclose(xy[edge], (5.0, 0.0)) and np.allclose(xy[floor], (6.5, 0.0))
    change = solver.bed_change
    with capsys.disabled():
        print('bed change at the upstream edge (5, 0) {:+.3e}, on the floor (6.5, 0) {:+.3e}'.format(change[edge], change[floor]))
    assert change[floor] < 0.0 < change[edge]
    assert solver.iteration == 48 and solver.fields.sediment_2d.dat.data_ro.min() > 0


@pytest.mark.parametrize('stepper', ['SSPRK33', 'ForwardEuler'])
def test_iterate_batches_equal_the_step_by_step_loop(stepper):
    """12 steps in batches of 3 (iterate) against the generator taken step by step: flow, sediment and bathymetry bit for bit"""
    mod = _example()
    res = []
    for batched in (True, False):
        solver, bed0, args = mod.setup(['--nx', '16', '--ny', '2', '--steps', '12', '--stepper', stepper])
        if batched:
            solver.iterate()
        else:
            for _ in solver.create_iterator():
                pass
        f = solver.fields
        res.append([f.uv_2d.dat.data_ro.copy(), f.elev_2d.dat.data_ro.copy(), f.sediment_2d.dat.data_ro.copy(),
                    f.bathymetry_2d.dat.data_ro.copy()])
        assert solver.iteration == 12 and np.abs(res[-1][3] - bed0).max() > 0 and np.isfinite(res[-1][2]).all()
    for a, b, what in zip(res[0], res[1], ('uv', 'elev', 'sediment', 'bathymetry')):
        assert np.array_equal(a, b), what


@pytest.mark.parametrize('stepper,per_stage', [('ForwardEuler', False), ('SSPRK33', True)])
def test_the_python_loop_equals_an_explicit_device_loop(stepper, per_stage):
    """The solver's step-by-step path (ForwardEuler sediment; SSPRK33 with a forcing callback, which takes the stages one by one)
    against the order written out with single device calls: flow stages, sediment_update, sediment stage(s), limiter, exner_step -
    flow, sediment and bathymetry bit for bit after 12 steps."""
    mod = _example()
    argv = ['--nx', '16', '--ny', '2', '--steps', '12', '--stepper', stepper]
    solver, bed0, args = mod.setup(argv)
    for _ in solver.create_iterator(update_forcings=(lambda t: None) if per_stage else None):
        pass
    f = solver.fields
    other, _, _ = mod.setup(argv)
    ti = other.timestepper
    dev, ts = ti.device, ti.tracers['sediment_2d']
    assert not ts.host_sediment and other.options.use_limiter_for_tracers
    ti.swe._sync_to_device()
    ts._sync_to_device()
    for _ in range(12):
        for i in range(3):
            dev.solve_stage(i)
        dev.sediment_update()
        if stepper == 'ForwardEuler':
            dev.tracer_forward_euler(ts.tid)
        else:
            for i in range(3):
                dev.tracer_solve_stage(ts.tid, i)
        dev.tracer_limit(ts.tid)
        dev.exner_step()
    uv, eta = dev.get_state()
    assert np.array_equal(f.uv_2d.dat.data_ro.reshape(uv.shape), uv) and np.array_equal(f.elev_2d.dat.data_ro.reshape(eta.shape), eta)
    sed = dev.tracer_get_state(ts.tid)
    assert np.array_equal(f.sediment_2d.dat.data_ro.reshape(sed.shape), sed)
    bed = dev.get_bathymetry()
    assert np.array_equal(f.bathymetry_2d.dat.data_ro, bed) and np.abs(bed - bed0).max() > 0


def test_host_fallback_on_a_real_device_equals_the_device_passes():
    """a device class that hides the sediment calls: the stepper evaluates HostSediment per stage.  Source, 'equilibrium' facets and
    Exner are the device's bits from the same planes; the planes differ by the rounding of the two math libraries, so the runs agree
    to a few times that bound (tests/test_gpu_sediment.py) and not bit for bit"""
    from thetis_amd.device import Swe2dDevice

    class HostFallbackDevice(Swe2dDevice):
        @property
        def sediment_set(self):
            raise AttributeError('sediment_set')
    mod = _example()
    argv = ['--nx', '16', '--ny', '2', '--steps', '6']
    res = []
    for cls in (None, HostFallbackDevice):
        import thetis_amd.solver2d as s2d
        orig = s2d.FlowSolver2d.__init__

        def init(self, *a, **kw):
            orig(self, *a, **kw)
            if cls is not None:
                self._device_cls = cls
        s2d.FlowSolver2d.__init__ = init
        try:
            solver, bed0, args = mod.setup(argv)
        finally:
            s2d.FlowSolver2d.__init__ = orig
        assert solver.timestepper.tracers['sediment_2d'].host_sediment == (cls is not None)
        solver.iterate()
        res.append((solver.fields.sediment_2d.dat.data_ro.copy(), solver.fields.bathymetry_2d.dat.data_ro.copy() - bed0))
    (sa, ba), (sb, bb) = res
    assert np.abs(sa - sb).max() <= 1e-11*np.abs(sa).max() and np.abs(ba - bb).max() <= 1e-11*np.abs(ba).max() and np.abs(ba).max() > 0
