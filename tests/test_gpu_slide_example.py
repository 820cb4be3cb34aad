"""examples/sediment_slide.py through FlowSolver2d on the device (400 triangles): iterate()'s batches equal the generator taken step by
step bit for bit, with flow and bedload and with the slide alone; the slide alone follows the numbers of HostSediment on the ramp;
with flow and bedload the largest angle falls and nothing is flagged or skipped."""
import importlib.util
import os

import numpy as np
import pytest

from slide_cases import RAMP_ANGLE
from test_gpu_slide import ALPHA_BOUND
from test_slide import ramp_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location('sediment_slide', os.path.join(ROOT, 'examples', 'sediment_slide.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('mode', [['--end', '0.03', '--export', '0.01'], ['--slide-only', '--end', '1.2', '--export', '0.4']])
def test_iterate_batches_equal_the_step_by_step_loop(mode):
    """a few batches (iterate) against the generator taken step by step: flow, bed, alpha, beta and the maximum angle bit for bit"""
    mod = _example()
    res = []
    for batched in (True, False):
        solver, bed0, args = mod.setup(mode)
        model = solver.sediment_model
        assert model.on_device and model.use_sediment_slide and model.use_bedload == ('--slide-only' not in mode)
        assert not hasattr(solver.fields, 'sediment_2d')
        assert model.max_slope_angle() == pytest.approx(RAMP_ANGLE, abs=1e-9)    # of the initial bed
        assert model.betaangle.dat.data_ro.max() == solver.timestepper.device.slide_max_angle()
        if batched:
            solver.iterate()
        else:
            n = sum(1 for _ in solver.create_iterator())
            assert n == solver.iteration
        f = solver.fields
        alpha, beta, _ = solver.timestepper.device.slide_read()
        assert np.array_equal(model.get_sediment_slide_term().dat.data_ro, alpha) and np.array_equal(model.betaangle.dat.data_ro, beta)
        assert alpha.min() < 0 and alpha.max() <= 0
        res.append([f.uv_2d.dat.data_ro.copy(), f.elev_2d.dat.data_ro.copy(), f.bathymetry_2d.dat.data_ro.copy(), alpha, beta,
                    np.array([model.max_slope_angle(), model.slide_flagged(), solver.iteration])])
        assert solver.iteration >= 12 and np.abs(res[-1][2] - bed0).max() > 0 and all(np.isfinite(a).all() for a in res[-1])
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_the_slide_alone_follows_the_host_numbers(capsys):
    """--slide-only, dt = 0.1, 200 steps: the angle printed at an export is that of the last pass, i.e. of the bed the last step
    started from.  The device's alpha differs from numpy's by at most ALPHA_BOUND of max |alpha| per pass (tests/test_gpu_slide.py) and
    the update is a contraction: the differences of the 200 passes add up at most, each at most ALPHA_BOUND of the angle."""
    mod = _example()
    solver = mod.main(['--slide-only', '--end', '20', '--export', '5'])
    out = capsys.readouterr().out
    assert out.count('largest slope angle') == 5
    want, flagged, drift = ramp_run(200)
    got = np.array(solver.angles)
    tol = 200*ALPHA_BOUND*RAMP_ANGLE
    with capsys.disabled():
        print('slide alone: angles {:}, largest difference from the host {:.3e} degrees (tolerance {:.3e})'.format(
            np.round(got, 4), np.abs(got - want[[0, 49, 99, 149, 199]]).max(), tol))
    assert np.abs(got - want[[0, 49, 99, 149, 199]]).max() <= tol
    assert (np.diff(got) < 0).all() and 24.5 < got[-1] < 25.0
    assert solver.sediment_model.slide_flagged() == 0 and solver.timestepper.device.exner_skipped() == 0
    assert solver.iteration == 200


def test_with_flow_and_bedload_the_angle_falls(capsys):
    """5 s of the example's 20 (about 2300 steps at the automatic step): over the first 2 s the bedload at the crest of the ramp lifts
    the largest angle by 3e-4 degrees before the slide takes it down - 26.541 degrees at 5 s, 25.62 at 20 s"""
    mod = _example()
    solver = mod.main(['--end', '5', '--export', '2.5'])
    out = capsys.readouterr().out
    assert out.count('largest slope angle') == 3 and 'bed change' in out
    model = solver.sediment_model
    with capsys.disabled():
        print('flow + bedload + slide: {:d} steps of {:.5f} s, angles {:}'.format(solver.iteration, solver.dt, np.round(solver.angles, 4)))
    assert solver.angles[0] == pytest.approx(RAMP_ANGLE, abs=1e-9) and solver.angles[-1] < solver.angles[0]
    assert model.slide_flagged() == 0 and solver.timestepper.device.exner_skipped() == 0
    qbx, qby = model.get_bedload_term()
    assert np.isfinite(qbx).all() and qbx.max() > 0 and np.abs(solver.bed_change).max() > 0
    u = solver.fields.uv_2d.dat.data_ro[:, 0]
    assert 0.2 < u.min() and u.max() < 0.8
