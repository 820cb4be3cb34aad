#!/usr/bin/env python
"""Cost of the Smagorinsky viscosity update (csrc/swe2d_smag.hip) on the cfg 2 channel, with the conventions of tools/cfgbench.py:
the step with a CG-P1 viscosity field, the step with the closure on top of it, and the two update kernels alone.
   python tools/smagbench.py            (SMAGBENCH_NX=1000: 1 M triangles)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cfgbench import timed                       # noqa: E402
from thetis_amd.device import Swe2dDevice        # noqa: E402
from thetis_amd.mesh import RectangleMesh        # noqa: E402


def main():
    nx = int(os.environ.get('SMAGBENCH_NX', '1000'))
    rng = np.random.default_rng(1234)
    mesh = RectangleMesh(nx, nx//2, 100e3, 50e3)
    n = mesh.num_cells
    cxy = mesh.cell_xy()
    eta = 0.5*np.exp(-((cxy[:, :, 0] - 50e3)**2 + (cxy[:, :, 1] - 25e3)**2)/(5e3)**2) + 1e-3*rng.uniform(-1, 1, size=(n, 3))
    uv = 1e-3*rng.uniform(-1, 1, size=(n, 3, 2))
    dt = 0.25*1000.0/nx
    dev = Swe2dDevice(mesh, np.full(mesh.num_vertices, 20.0), dt)
    dev.set_state(uv, eta)
    # the element size of a uniform mesh (the CG-P1 projection of a constant is that constant)
    he = np.full(mesh.num_vertices, float(np.sqrt(mesh.cell_areas()[0])))
    nu = 10.0 + rng.uniform(size=mesh.num_vertices)
    out = {'n_cells': n}
    dev.set_viscosity(nu)
    out['us_per_step_viscosity_field'] = 1e6*timed(dev, dev.advance, 50)
    t_stage = timed(dev, lambda k: [dev.solve_stage(0) for _ in range(k)], 50)
    out['us_per_stage_launch_viscosity_field'] = 1e6*t_stage
    dev.set_state(uv, eta)
    dev.smag_set(0.1, he)
    out['us_per_step_smagorinsky'] = 1e6*timed(dev, dev.advance, 50)
    dev.set_state(uv, eta)
    out['us_per_update_alone'] = 1e6*timed(dev, lambda k: [dev.smag_update() for _ in range(k)], 50)
    out['update_over_stage_launch'] = out['us_per_update_alone']/out['us_per_stage_launch_viscosity_field']
    dev.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
