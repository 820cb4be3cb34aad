"""Shared builders of the atmospheric-forcing tests (tests/test_atm_forcing.py on the CPU, tests/test_gpu_atm.py on the GPU): the
8 x 4 meshes of tests/tide_cases.py plus a 20 x 7 triangle mesh of 280 cells - the smallest with a second, partial workgroup, a plane
stride (512) other than the cell count and a vertex count (168) other than both -, seeded records that are smooth in space, the solver
set-up on a closed basin, and the two-rank scenario for dist_worker / spmd_cases."""
import numpy as np

from thetis_amd import AtmosphericForcing, Constant, Function, get_functionspace, solver2d
from thetis_amd.forcing import wind_drag_coefficient
from thetis_amd.mesh import Mesh2d, _grid_cells
from tide_cases import LX, LY, tide_mesh

EPS = float(np.finfo(np.float64).eps)
METHODS = ('LargeYeager2009', 'LargePond1981', 'SmithBanke1975')
# snapshot times: two, and five with uneven spacing; both cover every stage time of the tests (up to 0.7 + 23*0.3 + 0.3 = 7.9)
TIMES = {2: np.array([0.0, 9.5]), 5: np.array([0.0, 1.1, 2.9, 4.0, 9.5])}
SWITCHES = (11.0, 33.0)


def atm_mesh(kind='triangles'):
    if kind != 'tri280':
        return tide_mesh(kind)
    xs, ys = np.linspace(0.0, LX, 21), np.linspace(0.0, LY, 8)
    xx, yy = np.meshgrid(xs, ys, indexing='ij')
    mesh = Mesh2d(np.stack([xx.ravel(), yy.ravel()], axis=1), _grid_cells(20, 7, 'left'),
                  marker_fn=lambda xm, ym: np.where(np.abs(xm) < 1e-6, 1, 2))
    assert mesh.num_cells == 280 and mesh.num_vertices == 168
    return mesh


def eval_times(times):
    """the first, an interior and the last snapshot time, and two times off the grid"""
    times = np.asarray(times)
    return [float(times[0]), float(times[len(times)//2]), float(times[-1]), 0.37*float(times[-1]), float(times[-1]) - 0.6]


def atm_tables(mesh, n_t=5, seed=0):
    """times (n_t,), wind_u, wind_v, pressure (n_t, n_vertices): a wind that vanishes exactly on x = 0 and grows to 38 .. 45 m/s at
    x = LX while it turns with y and from snapshot to snapshot, and a pressure low that crosses the basin"""
    rng = np.random.default_rng(300 + seed)
    times = TIMES[n_t]
    x, y = mesh.vertex_xy[:, 0]/LX, mesh.vertex_xy[:, 1]/LY
    top = np.concatenate([[45.0], rng.uniform(38.0, 44.0, size=n_t - 1)])
    theta = 0.4*np.arange(n_t) + rng.uniform(0.0, 0.2, size=n_t)
    u = np.stack([top[k]*x*np.cos(theta[k] + 1.3*y) for k in range(n_t)])
    v = np.stack([top[k]*x*np.sin(theta[k] + 1.3*y)*(1.0 - 0.1*y) for k in range(n_t)])
    xc = np.linspace(0.1, 0.9, n_t)
    p = np.stack([101325.0 - 2500.0*np.exp(-((x - xc[k])**2 + (y - 0.5)**2)/0.08) for k in range(n_t)])
    return times, u, v, p


def make_atm(mesh, n_t=5, method='LargeYeager2009', wind=True, pressure=True, seed=0, units='pa', check_times=None):
    """an AtmosphericForcing on fresh fields of ``mesh``.  Asserts what the bit-for-bit comparisons rest on: the wind is exactly zero
    at a vertex, its speeds span 0 .. 45 m/s, and no speed - at ``check_times``, by default ``eval_times`` - lies within 1e-6 of a
    switch of C_D (11, 33 m/s), where a last-place difference in the speed would pick the other branch"""
    times, u, v, p = atm_tables(mesh, n_t, seed)
    if units == 'hpa':
        p = p/100.0
    ws = Function(get_functionspace(mesh, 'CG', 1, vector=True), name='wind_stress') if wind else None
    pa = Function(get_functionspace(mesh, 'CG', 1), name='atm_pressure') if pressure else None
    f = AtmosphericForcing(ws, pa, times, u if wind else None, v if wind else None, p if pressure else None, method=method,
                           pressure_units=units)
    if wind:
        speeds = []
        for t in (eval_times(times) if check_times is None else check_times):
            j, alpha = f.bracket(t)
            ui, vi = (1.0 - alpha)*f.wind_u[j] + alpha*f.wind_u[j + 1], (1.0 - alpha)*f.wind_v[j] + alpha*f.wind_v[j + 1]
            speeds.append(np.sqrt(ui*ui + vi*vi))
        m = np.concatenate(speeds)
        assert (m == 0.0).any() and m.max() > 33.5 and ((m > 0.0) & (m < 11.0)).any() and ((m > 11.0) & (m < 33.0)).any()
        assert m.max() <= 45.0
        for sw in SWITCHES:
            assert np.abs(m - sw).min() > 1e-6, 'a speed within 1e-6 of the switch at {:} m/s'.format(sw)
    return f


def stress_sensitivity(method, speeds):
    """max over ``speeds`` (> 0) of |tau(m') - tau(m)|/(eps |tau(m)|), m' the doubles next to m on either side, with
    tau(m) = C_D(m)*rho_air*m evaluated as compute_wind_stress does: how many eps one ulp of the speed moves the stress by"""
    m = np.asarray(speeds, dtype=np.float64)
    m = m[m > 0.0]

    def tau(mm):
        return wind_drag_coefficient(mm, method)*1.22*mm
    t0 = tau(m)
    d = np.maximum(np.abs(tau(np.nextafter(m, np.inf)) - t0), np.abs(tau(np.nextafter(m, -np.inf)) - t0))
    return float((d/(EPS*np.abs(t0))).max())


def make_solver(mesh, wind_stress=None, atmospheric_pressure=None, dt=0.3, n_steps=6, n_export=None, stepper='SSPRK33', outdir=None,
                tracer=False):
    """a FlowSolver2d on the closed basin ``mesh`` with the two option values as given"""
    P1 = get_functionspace(mesh, 'CG', 1)
    bath = Function(P1).interpolate(lambda x, y: 12.0 - 3.0*x/LX + 0.5*np.sin(y/900.0))
    s = solver2d.FlowSolver2d(mesh, bath)
    o = s.options
    o.swe_timestepper_type = stepper
    o.swe_timestepper_options.use_automatic_timestep = False
    o.timestep = dt
    o.simulation_export_time = (n_export or n_steps)*dt
    o.simulation_end_time = (n_steps - 0.5)*dt
    o.no_exports = True
    if outdir is not None:
        o.output_directory = outdir
    o.manning_drag_coefficient = Constant(0.02)
    o.wind_stress = wind_stress
    o.atmospheric_pressure = atmospheric_pressure
    if tracer:
        o.add_tracer_2d('tracer_2d', 'Depth averaged tracer', 'Tracer2d', source=None, diffusivity=None)
        o.tracer_timestepper_type = stepper
        o.tracer_timestepper_options.use_automatic_timestep = False
    kw = {'tracer': Function(P1).interpolate(lambda x, y: 1.0 + (x > 0.5*LX))} if tracer else {}
    s.assign_initial_conditions(elev=Function(P1).interpolate(lambda x, y: 0.1*np.cos(np.pi*x/LX)), **kw)
    return s


# ---- the scenario of the two-rank test: run through dist_worker.spmd_worker / spmd_cases.run under the name 'atm'
def _atm_case(outdir, cpu=False):
    mesh = atm_mesh('triangles')
    f = make_atm(mesh, n_t=5)
    s = make_solver(mesh, f, f, dt=0.3, n_steps=20, n_export=10, outdir=outdir)
    s.iterate()
    return s


def atm_worker(rank, world, port, out_dir, name, cpu, env):
    import dist_worker
    import spmd_cases
    spmd_cases.CASES['atm'] = _atm_case
    dist_worker.spmd_worker(rank, world, port, out_dir, name, cpu=cpu, env=env)


def run_atm_ranks(world, out_dir, timeout=300):
    """``dist_worker.run_spmd`` for the scenario of this file: the per-rank result dictionaries of ``spmd_cases.run``"""
    import multiprocessing as mp
    import os
    import pickle
    import socket
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=atm_worker, args=(r, world, port, out_dir, 'atm', False, None)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
    for p in procs:
        if p.is_alive():
            for q in procs:
                if q.is_alive():
                    q.terminate()
            raise RuntimeError('atm worker timed out')
        assert p.exitcode == 0, 'atm worker failed with exit code {:}'.format(p.exitcode)
    out = []
    for r in range(world):
        with open(os.path.join(out_dir, 'res_w{:d}_r{:d}.pkl'.format(world, r)), 'rb') as f:
            out.append(pickle.load(f))
    return out
