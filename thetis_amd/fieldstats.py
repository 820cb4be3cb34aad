"""
Running statistics of whole fields over every sampled step: extrema, means and tidal harmonics of the elevation, maximum and mean
speed, the residual current and the mean of |u|^3 - at every DG node, accumulated on the device (csrc/swe2d_stats.hip).

    cb = FieldStatisticsCallback(solver_obj, harmonics={'M2': 1.405189e-4, 'S2': 1.454441e-4}, every=10)
    solver_obj.add_callback(cb, eval_interval='timestep')
    solver_obj.iterate()
    r = cb.result()          # r['elev_amp']['M2'], r['speed_max'], r['uv_mean'], ...

The reference has no such callback: its ``AccumulatorCallback`` (thetis/callback.py:588) integrates a scalar in time, not fields.

One sample updates, per node and left to right (e, u, v: the node's elevation and velocity),

    q = u*u + v*v            s = sqrt(q)
    e_min = e < e_min ? e : e_min        e_max = e > e_max ? e : e_max        q_max = q > q_max ? q : q_max
    e_sum += e    u_sum += u    v_sum += v    s_sum += s    s3_sum += q*s
    C_k += e*cos(omega_k t)        S_k += e*sin(omega_k t)

The weights cos / sin(omega_k t) depend on time only: the host forms them with numpy and hands them to the append call, so the
device evaluates no transcendental.  The host also keeps the small normal matrix W = sum w w^T, w = [1, cos omega_k t, sin omega_k t];
the harmonic constants follow at the end from W x = [e_sum, C_k, S_k] for all nodes at once.
"""
import os

import numpy as np

from . import _lib
from .callback import DiagnosticCallback
from .forcing import HarmonicTidalForcing
from .function import Function
from .timeintegrator import StepConsumer

__all__ = ['FieldStatisticsCallback', 'HostFieldStats', 'harmonic_weights', 'solve_harmonics', 'COND_LIMIT', 'ACCUMULATORS']

ACCUMULATORS = ('e_min', 'e_max', 'q_max', 'e_sum', 'u_sum', 'v_sum', 's_sum', 's3_sum')      # then C_0, S_0, C_1, S_1, ...

# The largest 2-norm condition number of W at which ``result()`` still solves for the harmonic constants.  The sums on the right
# hand side carry a relative rounding error of about n*eps (plain summation of n samples), the solve returns it amplified by
# cond(W): at the limit a record of 1e5 samples (n*eps ~ 1e-11) still gives amplitudes to 1e-5 of the signal, the resolution of a
# tide table.  Beyond the rounding, whatever part of the signal is NOT harmonic (wind, river flow, shallow-water overtides) comes
# back amplified by about sqrt(cond(W)) - three orders of magnitude at the limit, so the "amplitudes" stop meaning anything.
# A record that resolves its constituents is far below: W/n tends to diag(1, 1/2, 1/2, ...), condition number 2; M2 + S2 over
# 3 days give 32, over 1 day 3e2, over 12 hours 7e3.  What the limit must catch is far above: fewer than 2K + 1 samples (W singular,
# > 1e16), M2 + S2 over 2 hours (2.6e10).
COND_LIMIT = 1.0e6


def harmonic_weights(omegas, t):
    """(2K,) = cos(omega_0 t), sin(omega_0 t), cos(omega_1 t), ...: what ``stats_append`` takes at time ``t``"""
    arg = np.asarray(omegas, dtype=np.float64)*float(t)
    w = np.empty(2*len(arg))
    w[0::2] = np.cos(arg)
    w[1::2] = np.sin(arg)
    return w


class HostFieldStats(object):
    """The accumulators of a statistics set in numpy, by the formulas of csrc/swe2d_stats.hip: the fallback of a device class
    without ``stats_append``."""

    def __init__(self, shape, n_constituents=0):
        self.K = int(n_constituents)
        self.acc = np.zeros((len(ACCUMULATORS) + 2*self.K,) + tuple(shape))
        self.reset()

    def reset(self):
        self.acc[...] = 0.0
        self.acc[0] = np.inf
        self.acc[1:3] = -np.inf
        self.n_samples = 0

    def append(self, uv, eta, weights=None):
        a = self.acc
        e = np.asarray(eta, dtype=np.float64).reshape(a.shape[1:])
        uv = np.asarray(uv, dtype=np.float64).reshape(a.shape[1:] + (2,))
        u, v = uv[..., 0], uv[..., 1]
        q = u*u + v*v
        s = np.sqrt(q)
        a[0] = np.where(e < a[0], e, a[0])
        a[1] = np.where(e > a[1], e, a[1])
        a[2] = np.where(q > a[2], q, a[2])
        a[3] = a[3] + e
        a[4] = a[4] + u
        a[5] = a[5] + v
        a[6] = a[6] + s
        a[7] = a[7] + q*s
        for k in range(self.K):
            a[8 + 2*k] = a[8 + 2*k] + e*float(weights[2*k])
            a[9 + 2*k] = a[9 + 2*k] + e*float(weights[2*k + 1])
        self.n_samples += 1

    def read(self):
        return self.acc.copy(), self.n_samples


def solve_harmonics(W, rhs):
    """x of W x = rhs ((2K + 1, ...) = [e_sum, C_0, S_0, ...]) -> (fit mean, amplitudes (K, ...), phases (K, ...)) in the convention
    of HarmonicTidalForcing, e = mean + sum_k A_k cos(omega_k t - phi_k).  ValueError when W is ill-conditioned (COND_LIMIT)."""
    W = np.asarray(W, dtype=np.float64)
    cond = np.linalg.cond(W) if np.isfinite(W).all() and W.any() else np.inf
    if not cond <= COND_LIMIT:
        raise ValueError('the harmonic fit is ill-conditioned: cond(W) = {:.3e} > {:.3e} - fewer than 2K + 1 = {:d} samples, or a '
                         'record too short to separate the constituents'.format(cond, COND_LIMIT, W.shape[0]))
    rhs = np.asarray(rhs, dtype=np.float64)
    x = np.linalg.solve(W, rhs.reshape(W.shape[0], -1)).reshape(rhs.shape)
    a, b = x[1::2], x[2::2]
    return x[0], np.hypot(a, b), np.arctan2(b, a)


class FieldStatisticsCallback(DiagnosticCallback, StepConsumer):
    """Running field statistics (see the module text).  Register with ``add_callback(cb, eval_interval='timestep')``: a sample is
    taken after a step when the solver's iteration count is a multiple of ``every`` and the time lies in [start_time, end_time].
    ``FlowSolver2d.iterate`` keeps its batches, and the steps between two samples go to the device in one call.

    ``harmonics``: {'M2': omega, ...} in rad/s, or a :class:`HarmonicTidalForcing` whose ``omegas`` are taken (named c0, c1, ...).
    A device class without statistics sets (the host stand-in of the tests) accumulates on the host from the fields' nodal values,
    step by step.  Several ranks: ``NotImplementedError`` at the first evaluation (the partitioned driver carries no statistics
    sets).  ``result()`` gives nodal arrays on P1DG_2d / P1DGv_2d, ``as_functions()`` the same as Functions; unless
    ``export_to_hdf5=False`` rank 0 rewrites ``<output_directory>/diagnostic_<name>.npz`` at every export - a full read-back of the
    accumulator planes each time (see ``export``)."""

    def __init__(self, solver_obj, harmonics=None, every=1, name='fieldstats', start_time=None, end_time=None,
                 export_to_hdf5=True, outputdir=None):
        super(FieldStatisticsCallback, self).__init__(solver_obj, append_to_log=False, start_time=start_time, end_time=end_time)
        self.name = name
        self.export_to_hdf5 = export_to_hdf5
        self.outputdir = outputdir
        self.every = int(every)
        if self.every < 1:
            raise ValueError('every must be >= 1')
        if isinstance(harmonics, HarmonicTidalForcing):
            harmonics = {'c{:d}'.format(k): float(om) for k, om in enumerate(harmonics.omegas)}
        self.constituents = list((harmonics or {}).keys())
        self.omegas = np.array([float(harmonics[c]) for c in self.constituents], dtype=np.float64)
        K = len(self.omegas)
        if K > _lib.MAX_TIDE_CONSTITUENTS:
            raise NotImplementedError('{:d} harmonic constituents: at most SWE2D_MAX_TIDE_CONSTITUENTS = {:d} are supported'.format(
                K, _lib.MAX_TIDE_CONSTITUENTS))
        self.W = np.zeros((2*K + 1, 2*K + 1))
        self.n_samples = 0
        self._set = None                        # (device, statistics id)
        self._host = None                       # HostFieldStats of a device class without statistics sets
        self._batch_iteration = 0

    # ---- where the accumulators live
    def _stepper(self):
        stepper = self.solver_obj.timestepper
        return getattr(stepper, 'swe', stepper)         # the coupled integrator (tracers) holds the shallow water stepper

    def _device_set(self):
        """(device, statistics id) on a device class with statistics sets, else None"""
        if getattr(self.solver_obj.comm, 'size', 1) > 1:
            raise NotImplementedError('FieldStatisticsCallback on several ranks: the partitioned driver does not carry statistics '
                                      'sets yet (run the statistics on one device)')
        dev = getattr(self._stepper(), 'device', None)
        if dev is None or not hasattr(dev, 'stats_append'):
            return None
        if self._set is not None and self._set[0] is not dev:
            raise RuntimeError('the time stepper changed its device under a FieldStatisticsCallback')
        if self._set is None:
            self._set = (dev, dev.stats_create(len(self.omegas)))
        return self._set

    def _due(self, iteration, t):
        return iteration % self.every == 0 and self.start_time <= t <= self.end_time

    def _count(self, t):
        """the host's part of a sample at time ``t``: W and the count.  Returns the weights of the append."""
        w2 = harmonic_weights(self.omegas, t)
        w = np.concatenate([[1.0], w2])
        self.W += np.outer(w, w)
        self.n_samples += 1
        return w2

    # ---- samples of a batch (FlowSolver2d.create_iterator; the stepper's advance_steps asks per step of the batch)
    def row_probe(self, n_rows):
        from .pointeval import device_ready
        if getattr(self.solver_obj.comm, 'size', 1) > 1 or not device_ready(self._stepper()):
            return None
        s = self._device_set()
        if s is None:
            return None
        self._batch_iteration = self.solver_obj.iteration
        return s[0], self

    def wants_append(self, k, t):
        """does step ``k`` of the batch, which ends at time ``t``, leave a sample?"""
        return self._due(self._batch_iteration + k + 1, t)

    def append(self, device, k, t):
        device.stats_append(self._set[1], self._count(t))

    # ---- one step at a time
    def evaluate(self, index=None):
        t = self.solver_obj.simulation_time
        s = self._device_set()
        if not self._due(self.solver_obj.iteration, t):
            return
        if s is not None:
            from .pointeval import device_ready
            if not device_ready(self._stepper()):
                raise RuntimeError('FieldStatisticsCallback evaluated between the stages of a step')
            s[0].stats_append(s[1], self._count(t))
            return
        f = self.solver_obj.fields
        self.add_host_sample(t, f.uv_2d.cell_node_values(), f.elev_2d.cell_node_values())

    def add_host_sample(self, t, uv, eta):
        """one sample at time ``t`` of the nodal values ``uv`` (..., 2) and ``eta`` (...), accumulated on the host (a callback whose
        device class has no statistics sets; never mixed with samples on the device)"""
        assert self._set is None, 'this callback accumulates on the device'
        eta = np.asarray(eta, dtype=np.float64)
        if self._host is None:
            self._host = HostFieldStats(eta.shape, len(self.omegas))
        self._host.append(uv, eta, self._count(t))

    def reset(self):
        self.W[...] = 0.0
        self.n_samples = 0
        if self._set is not None:
            self._set[0].stats_reset(self._set[1])
        if self._host is not None:
            self._host.reset()

    # ---- results
    def accumulators(self):
        """((8 + 2K, N, k) accumulators in the order of ACCUMULATORS then C_0, S_0, ..., samples); synchronises once"""
        if self._set is not None:
            acc, n = self._set[0].stats_read(self._set[1])
        elif self._host is not None:
            acc, n = self._host.read()
        else:
            acc, n = HostFieldStats((1, 1), len(self.omegas)).read()
        assert n == self.n_samples, 'the statistics set holds {:d} samples, the host counted {:d}'.format(n, self.n_samples)
        return acc, n

    def result(self, fit=True):
        """dict of nodal arrays: elev_min, elev_max, elev_mean, speed_max, speed_mean, speed_cubed_mean (N*k,), uv_mean (N*k, 2),
        and - ``fit`` - elev_amp[name], elev_phase[name], elev_fit_mean from the least-squares fit of
        mean + sum A cos(omega t - phi).  ValueError without samples or when the fit is ill-conditioned."""
        if self.n_samples == 0:
            raise ValueError('no samples yet: cond(W) = inf')
        acc, n = self.accumulators()
        a = acc.reshape(acc.shape[0], -1)
        out = {'elev_min': a[0], 'elev_max': a[1], 'elev_mean': a[3]/n, 'speed_max': np.sqrt(a[2]), 'speed_mean': a[6]/n,
               'speed_cubed_mean': a[7]/n, 'uv_mean': np.stack([a[4]/n, a[5]/n], axis=1)}
        if fit:
            mean, amp, phase = solve_harmonics(self.W, np.concatenate([a[3:4], a[8:]]))
            out['elev_fit_mean'] = mean
            out['elev_amp'] = {c: amp[k] for k, c in enumerate(self.constituents)}
            out['elev_phase'] = {c: phase[k] for k, c in enumerate(self.constituents)}
        return out

    def as_functions(self, fit=True):
        fs = self.solver_obj.function_spaces

        def func(name, v):
            return Function(fs.P1DGv_2d if v.ndim == 2 else fs.P1DG_2d, name=name).assign(v)
        out = {}
        for key, v in self.result(fit=fit).items():
            out[key] = {c: func('{:}_{:}'.format(key, c), x) for c, x in v.items()} if isinstance(v, dict) else func(key, v)
        return out

    def __call__(self):
        return (self.n_samples,)

    def message_str(self, *values):
        return '{:}: {:d} samples'.format(self.name, values[0])

    def export(self):
        """rank 0 rewrites diagnostic_<name>.npz with the statistics so far (without the harmonic constants while the record is too
        short to give them).  This is a ``result()``: one synchronisation, a read-back of all 8 + 2K accumulator planes (8 B per
        node and accumulator - 1 M triangles with K = 8: 576 MB) and the fit, at EVERY export of the solver; pass
        ``export_to_hdf5=False`` and call ``result()`` once at the end where the exports are frequent."""
        if not self.export_to_hdf5 or getattr(self.solver_obj.comm, 'rank', 0) != 0 or self.n_samples == 0:
            return
        try:
            r = self.result()
        except ValueError:
            r = self.result(fit=False)
        data = {'n_samples': np.array(self.n_samples), 'constituents': np.array(self.constituents), 'omegas': self.omegas}
        for key, v in r.items():
            if isinstance(v, dict):
                for c, x in v.items():
                    data['{:}_{:}'.format(key, c)] = x
            else:
                data[key] = v
        outdir = self.outputdir or self.solver_obj.options.output_directory
        os.makedirs(outdir, exist_ok=True)
        path = os.path.join(outdir, 'diagnostic_{:}.npz'.format(self.name))
        tmp = path + '.tmp.npz'
        np.savez(tmp, **data)
        os.replace(tmp, path)
