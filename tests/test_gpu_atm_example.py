"""examples/storm_surge.py at reduced size: a finite surge of the order the pressure low alone would raise."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_storm_surge_example(hip_lib):
    r = subprocess.run([sys.executable, os.path.join('examples', 'storm_surge.py'), '--nx', '16', '--ny', '8', '--t-end', '3600',
                        '--snapshots', '5'], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    w = r.stdout.strip().splitlines()[-1].split()
    assert w[0] == 'steps' and int(w[1]) >= 10
    eta, ib, finite = float(w[5]), float(w[w.index('inverse_barometer') + 1]), int(w[-1])
    print(r.stdout.strip().splitlines()[-1])
    # the inverse-barometer estimate dp/(rho0 g) = 0.41 m is what the low alone raises at rest; the wind adds to it, a low that
    # moves has not had the time to raise all of it: a non-trivial surge is above a tenth of the estimate, a sane one below ten times
    assert finite == 1 and np.isfinite(eta) and 0.1*ib < eta < 10.0*ib
