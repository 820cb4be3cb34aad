"""Storm surge in a closed basin: a synthetic pressure low with its cyclonic wind field crosses the basin from west to east.

The snapshots of 10 m wind and mean-sea-level pressure are tables on the mesh vertices; the ``AtmosphericForcing`` built from them is
given ITSELF as ``options.wind_stress`` and ``options.atmospheric_pressure``, so the device interpolates the record and forms the wind
stress in front of every Runge-Kutta stage and ``iterate()`` keeps its batches.  Prints the largest |elevation| reached
next to the inverse-barometer estimate dp/(rho0 g).

    python examples/storm_surge.py [--nx 60 --ny 30 --t-end 7200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from thetis_amd import AtmosphericForcing, Constant, Function, RectangleMesh, get_functionspace, solver2d  # noqa: E402

LX, LY, DEPTH = 300e3, 150e3, 20.0
DP, RADIUS, V_MAX = 4000.0, 40e3, 30.0          # pressure deficit [Pa], radius of maximum wind [m], maximum wind [m/s]


def storm(x, y, xc, yc):
    """wind (u, v) and pressure of a low centred at (xc, yc): a Rankine-like vortex, anticlockwise"""
    dx, dy = x - xc, y - yc
    r = np.sqrt(dx*dx + dy*dy)
    speed = V_MAX*(r/RADIUS)*np.exp(0.5*(1.0 - (r/RADIUS)**2))
    rr = np.where(r > 0.0, r, 1.0)
    return -speed*dy/rr, speed*dx/rr, 101325.0 - DP*np.exp(-0.5*(r/RADIUS)**2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nx', type=int, default=60)
    ap.add_argument('--ny', type=int, default=30)
    ap.add_argument('--t-end', type=float, default=7200.0)
    ap.add_argument('--snapshots', type=int, default=9)
    args = ap.parse_args()
    mesh = RectangleMesh(args.nx, args.ny, LX, LY)
    P1 = get_functionspace(mesh, 'CG', 1)
    P1v = get_functionspace(mesh, 'CG', 1, vector=True)
    x, y = mesh.vertex_xy.T
    # the low travels from x = 0.2 LX to 0.8 LX over the run; snapshots every t_end/(n - 1)
    times = np.linspace(0.0, args.t_end, args.snapshots)
    snaps = [storm(x, y, (0.2 + 0.6*t/args.t_end)*LX, 0.5*LY) for t in times]
    forcing = AtmosphericForcing(Function(P1v, name='wind_stress'), Function(P1, name='atm_pressure'), times,
                                 np.stack([s[0] for s in snaps]), np.stack([s[1] for s in snaps]), np.stack([s[2] for s in snaps]))
    s = solver2d.FlowSolver2d(mesh, Function(P1).assign(DEPTH))
    o = s.options
    o.swe_timestepper_type = 'SSPRK33'
    o.swe_timestepper_options.use_automatic_timestep = False
    dx = min(LX/args.nx, LY/args.ny)
    n_steps = int(np.ceil(args.t_end/(0.1*dx/np.sqrt(9.81*DEPTH))))        # explicit: well below the gravity-wave limit
    o.timestep = args.t_end/n_steps
    o.simulation_export_time = args.t_end/4.0
    o.simulation_end_time = args.t_end - 0.5*o.timestep
    o.no_exports = True
    o.quadratic_drag_coefficient = Constant(2.5e-3)
    o.wind_stress = forcing
    o.atmospheric_pressure = forcing
    s.assign_initial_conditions(elev=Constant(0.0))
    peak = [0.0]
    s.iterate(export_func=lambda: peak.__setitem__(0, max(peak[0], float(np.abs(s.fields.elev_2d.dat.data_ro).max()))))
    eta = s.fields.elev_2d.dat.data_ro
    uv = s.fields.uv_2d.dat.data_ro
    ib = DP/(1000.0*9.81)
    print('steps {:d} dt {:.3f} max|eta| {:.4f} m (peak at the exports {:.4f}) max|u| {:.4f} m/s inverse_barometer {:.4f} m finite {:d}'.format(
        s.iteration, o.timestep, float(np.abs(eta).max()), peak[0], float(np.abs(uv).max()), ib,
        int(np.isfinite(eta).all() and np.isfinite(uv).all())))


if __name__ == '__main__':
    main()
