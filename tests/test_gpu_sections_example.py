"""examples/strait_transport.py through FlowSolver2d on the device, on a reduced mesh and with a short tidal period: it runs, the
transports are finite, flood and ebb change sign at the throat, and the batched run prints the lines of the step-by-step loop."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = ['--nx', '16', '--ny', '4', '--period', '1800', '--periods', '1.5', '--every', '5']


def _example():
    spec = importlib.util.spec_from_file_location('strait_transport', os.path.join(ROOT, 'examples', 'strait_transport.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_strait_example(capsys):
    mod = _example()
    solver, cb = mod.main(ARGV)
    batched = capsys.readouterr().out
    r = cb.result()
    n = solver.iteration//5
    assert n > 20 and r['transport'].shape == (n, 2) and r['tracer_transport'].shape == (n, 2, 1)
    for key in ('transport', 'area', 'tracer_transport', 'cumulative_volume'):
        assert np.isfinite(r[key]).all(), key
    assert not r['n_unsummable'].any() and (r['area'] > 0.0).all()
    throat, inlet = r['transport'][:, 0], r['transport'][:, 1]
    assert throat.max() > 0.0 > throat.min()                 # flood into the basin, ebb out of it
    assert inlet.min() < 0.0 < inlet.max()                   # the boundary counts along the outward normal
    # the throat is half as wide as the channel (the transect's ends outside the mesh are dropped)
    assert abs(r['length'][0] - 0.5*mod.LY) < 1e-6*mod.LY and abs(r['length'][1] - mod.LY) < 1e-9*mod.LY
    lines = [l for l in batched.splitlines() if l.startswith(('steps', 'throat', 'open'))]
    assert len(lines) == 3 and 'tidal prism' in lines[1]
    mod.main(ARGV + ['--step-loop'])
    stepped = [l for l in capsys.readouterr().out.splitlines() if l.startswith(('steps', 'throat', 'open'))]
    assert stepped == lines
