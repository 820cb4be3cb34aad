"""
Run-time checks hooked into the time loop.  The reference has a general diagnostics framework (thetis/callback.py); the 2D
explicit path only ever registers three checks from ``FlowSolver2d.iterate`` (solver2d.py:1034-1059) - volume, tracer mass,
tracer over/undershoot - and all three are reductions the device already provides (``swe2d_diagnostics``,
``swe2d_tracer_diagnostics``).  So this module is one small class built around a device reduction, plus the registry the
solver iterates over; the reference's class names are kept as constructors so that user scripts written against
``thetis.callback`` (``VolumeConservation2DCallback(solver_obj, ...)``, ``solver_obj.add_callback(cb, 'export')``,
``solver_obj.callbacks['export']['volume2d']()``) keep working.  HDF5 sinks are I/O and out of scope; the detectors write .npz
files instead (``DetectorsCallback``).
"""
import os

import numpy as np

from .log import print_output
from .pointeval import PointNotInDomainError, select_and_move_detectors  # noqa: F401  (exported with the callbacks)

__all__ = ['CallbackManager', 'DiagnosticCallback', 'ScalarConservationCallback', 'MinMaxConservationCallback', 'DeviceCheck',
           'VolumeConservation2DCallback', 'TracerMassConservation2DCallback',
           'ConservativeTracerMassConservation2DCallback', 'TracerOvershootCallBack', 'DetectorsCallback', 'TimeSeriesCallback2D',
           'PointNotInDomainError', 'select_and_move_detectors', 'FieldStatisticsCallback', 'ParticleTrackerCallback',
           'SectionTransportCallback']


def __getattr__(name):
    # (thetis_amd/fieldstats.py, thetis_amd/particles.py and thetis_amd/sections.py build on DiagnosticCallback below: resolved on first use)
    if name == 'FieldStatisticsCallback':
        from .fieldstats import FieldStatisticsCallback
        return FieldStatisticsCallback
    if name == 'ParticleTrackerCallback':
        from .particles import ParticleTrackerCallback
        return ParticleTrackerCallback
    if name == 'SectionTransportCallback':
        from .sections import SectionTransportCallback
        return SectionTransportCallback
    raise AttributeError('module {!r} has no attribute {!r}'.format(__name__, name))


class CallbackManager(dict):
    """``manager[mode][name] -> check``; modes are 'export' and 'timestep'."""

    def __missing__(self, mode):
        self[mode] = {}
        return self[mode]

    def add(self, check, mode):
        self[mode][check.name] = check

    def evaluate(self, mode, index=None):
        for name in sorted(self[mode]):
            self[mode][name].evaluate(index=index)

    def export(self):
        """the file sinks (DetectorsCallback), at every export of the solver"""
        for mode in sorted(self):
            for name in sorted(self[mode]):
                if hasattr(self[mode][name], 'export'):
                    self[mode][name].export()


class DiagnosticCallback(object):
    """The extension point user scripts subclass (thetis/callback.py:162-301): a subclass provides ``name``, ``__call__()``
    (returns the tuple of diagnostic values; any reduction over ranks happens in there) and ``message_str(*values)``;
    ``evaluate`` is what the time loop calls - inside the optional [start_time, end_time] window it evaluates, keeps the
    values in ``history`` and prints the message.  ``variable_names`` is accepted for compatibility; there is no HDF5 sink on
    this path (``export_to_hdf5``, ``outputdir``, ``attrs``, ``array_dim``, ``hdf5_dtype``, ``include_time`` are taken and ignored)."""
    name = 'diagnostic'
    variable_names = ()

    def __init__(self, solver_obj, append_to_log=True, start_time=None, end_time=None, **ignored):
        self.solver_obj = solver_obj
        self.append_to_log = append_to_log
        self.start_time = -float('inf') if start_time is None else start_time
        self.end_time = float('inf') if end_time is None else end_time
        self.history = []

    def __call__(self):
        raise NotImplementedError('a DiagnosticCallback subclass must implement __call__')

    def message_str(self, *values):
        return '{:} diagnostic'.format(self.name)

    def push_to_log(self, time, values):
        print_output(self.message_str(*values))

    def evaluate(self, index=None):
        t = self.solver_obj.simulation_time
        if t < self.start_time or t > self.end_time:
            return
        values = self()
        values = tuple(values) if isinstance(values, (tuple, list)) else (values,)
        self.history.append((t,) + values)
        if self.append_to_log:
            self.push_to_log(t, values)


class ScalarConservationCallback(DiagnosticCallback):
    """``scalar_callback()`` against its first value: returns (value, relative difference) (thetis/callback.py:304-332)."""
    variable_names = ['integral', 'relative_difference']

    def __init__(self, scalar_callback, solver_obj, **kwargs):
        super(ScalarConservationCallback, self).__init__(solver_obj, **kwargs)
        self.scalar_callback = scalar_callback
        self.initial_value = None

    def __call__(self):
        now = self.scalar_callback()
        if self.initial_value is None:
            self.initial_value = now
        return now, (now - self.initial_value)/self.initial_value

    def message_str(self, *values):
        return '{0:s} rel. error {1:11.4e}'.format(self.name, values[1])


class MinMaxConservationCallback(DiagnosticCallback):
    """``minmax_callback()`` -> (min, max) against the first pair: returns (min, max, undershoot <= 0, overshoot >= 0)
    (thetis/callback.py:415-460)."""
    variable_names = ['min_value', 'max_value', 'undershoot', 'overshoot']

    def __init__(self, minmax_callback, solver_obj, **kwargs):
        super(MinMaxConservationCallback, self).__init__(solver_obj, **kwargs)
        self.minmax_callback = minmax_callback
        self.initial_value = None

    def __call__(self):
        lo, hi = self.minmax_callback()
        if self.initial_value is None:
            self.initial_value = (lo, hi)
        return lo, hi, min(lo - self.initial_value[0], 0.0), max(hi - self.initial_value[1], 0.0)

    def message_str(self, *values):
        return '{0:s} {1:g} {2:g}'.format(self.name, values[2], values[3])


class DeviceCheck(object):
    """A named reduction of the device-resident state compared with its value at the first evaluation.

    ``kind='conserved'``: ``reduce()`` returns a scalar; a call returns (value, relative drift).
    ``kind='bounds'``:    ``reduce()`` returns (min, max); a call returns (min, max, undershoot <= 0, overshoot >= 0)."""

    def __init__(self, name, solver_obj, reduce, kind='conserved', append_to_log=True, start_time=None, end_time=None,
                 **ignored):                       # export_to_hdf5, outputdir, ...: no file sinks on this path
        assert kind in ('conserved', 'bounds')
        self.name, self.solver_obj, self.kind = name, solver_obj, kind
        self._reduce = reduce
        self._log = append_to_log
        self._window = (-float('inf') if start_time is None else start_time, float('inf') if end_time is None else end_time)
        self.reference_value = None
        self.history = []

    @property
    def initial_value(self):                   # the reference's attribute name (callback.py:320)
        return self.reference_value

    @initial_value.setter
    def initial_value(self, value):
        self.reference_value = value

    def __call__(self):
        now = self._reduce()
        if self.reference_value is None:
            self.reference_value = now
        ref = self.reference_value
        if self.kind == 'conserved':
            return now, (now - ref)/ref
        lo, hi = now
        return lo, hi, min(lo - ref[0], 0.0), max(hi - ref[1], 0.0)

    def message_str(self, *values):
        if self.kind == 'conserved':
            return '{0:s} rel. error {1:11.4e}'.format(self.name, values[1])
        return '{0:s} {1:g} {2:g}'.format(self.name, values[2], values[3])

    def evaluate(self, index=None):
        t = self.solver_obj.simulation_time
        if not self._window[0] <= t <= self._window[1]:
            return
        values = self()
        self.history.append((t,) + tuple(values))
        if self._log:
            print_output(self.message_str(*values))


def _tracer_reduction(solver_obj, tracer_name, pick):
    def reduce():
        ts = solver_obj.timestepper.tracers[tracer_name]
        ts._sync_to_device()
        return pick(ts.device.tracer_diagnostics(ts.tid))        # {int T*H dx, int T dx, min, max}
    return reduce


def VolumeConservation2DCallback(solver_obj, **kwargs):
    """int (eta + h) dx (callback.py:350-364, utility.py:421-425)"""
    return DeviceCheck('volume2d', solver_obj, lambda: float(solver_obj.timestepper.diagnostics()[2]), **kwargs)


def TracerMassConservation2DCallback(tracer_name, solver_obj, **kwargs):
    """int T*H dx of a depth-averaged tracer (callback.py:366-389)"""
    return DeviceCheck(tracer_name + ' mass', solver_obj, _tracer_reduction(solver_obj, tracer_name, lambda d: float(d[0])), **kwargs)


def ConservativeTracerMassConservation2DCallback(tracer_name, solver_obj, **kwargs):
    """int q dx of a depth-integrated tracer (callback.py:392-412)"""
    return DeviceCheck(tracer_name + ' mass', solver_obj, _tracer_reduction(solver_obj, tracer_name, lambda d: float(d[1])), **kwargs)


def TracerOvershootCallBack(tracer_name, solver_obj, **kwargs):
    """nodal min/max of a tracer against their initial values (callback.py:463-483)"""
    return DeviceCheck(tracer_name + ' overshoot', solver_obj,
                       _tracer_reduction(solver_obj, tracer_name, lambda d: (float(d[2]), float(d[3]))), kind='bounds', **kwargs)


class DetectorsCallback(DiagnosticCallback):
    """Fields at fixed points - tide gauges, probes (thetis/callback.py:486-583).  A call returns (detectors, sum of the field
    dimensions); ``history`` holds (time, that array) per evaluation.  The points are located once, on the host
    (thetis_amd/pointeval.py); the solver's device-resident fields (uv_2d, elev_2d, tracers) are then gathered on the device by one
    probe set (csrc/swe2d_probe.hip) - never by copying the state to the host.  Registered for every time step, such detectors keep
    ``FlowSolver2d.iterate`` batching its steps: the device appends one row after every step and the rows are read at the end of the
    batch (``take_row``).  There is no HDF5 here: unless ``export_to_hdf5=False``, rank 0 rewrites
    ``<output_directory>/diagnostic_<name>.npz`` at every export, with the datasets and attributes of the reference's file (time (n, 1),
    one (n, sum of dims) array per detector name, field_names, field_dims, detector_names, detector_xy)."""

    def __init__(self, solver_obj, detector_locations, field_names, name, detector_names=None, **kwargs):
        kwargs.setdefault('append_to_log', False)       # printing every detector is not a useful default (the reference's choice)
        self.export_to_hdf5 = kwargs.pop('export_to_hdf5', True)
        self.outputdir = kwargs.pop('outputdir', None)
        super(DetectorsCallback, self).__init__(solver_obj, **kwargs)
        self.field_names = list(field_names)
        self.field_dims = [2 if solver_obj.fields[f].function_space().vector else 1 for f in self.field_names]
        self.detector_locations = [[float(v) for v in loc] for loc in detector_locations]
        n = len(self.detector_locations)
        if detector_names is None:
            fill = len(str(n))
            self.detector_names = ['detector{:0{fill}d}'.format(i, fill=fill) for i in range(n)]
        else:
            assert n == len(detector_names), 'Different number of detector locations and names'
            self.detector_names = list(detector_names)
        self._name = name
        self._loc = None
        self._probe = None                              # (device, probe id, row capacity)
        self._eval_func = None                          # TimeSeriesCallback2D(eval_func=...): host evaluation

    @property
    def name(self):
        return self._name

    @property
    def variable_names(self):
        return self.detector_names

    def _locate(self):
        if self._loc is None:
            from .pointeval import PointLocator
            loc = PointLocator(self.solver_obj.mesh2d, self.detector_locations)
            loc.check(self.detector_names)
            self._loc = loc
        return self._loc

    def _values_per_field(self, values):
        i, out = 0, []
        for dim in self.field_dims:
            out.append(values[i:i + dim])
            i += dim
        return out

    def message_str(self, *args):
        return '\n'.join(
            'In {}: '.format(name) + ', '.join(
                '{}={}'.format(field_name, field_val) for field_name, field_val in zip(self.field_names, self._values_per_field(values)))
            for name, values in zip(self.detector_names, args))

    # ---- the device path
    def _device_fields(self):
        """[(stepper, probe field code)] when every field lives on one device handle, else None"""
        out = []
        for f in self.field_names:
            func = self.solver_obj.fields[f]
            d = getattr(func, '_device_field', None)
            fs = func.function_space()
            if d is None or fs.family != 'DG' or fs.degree != 1:
                return None
            out.append(d)
        if len(set(id(s.device) for s, _ in out)) != 1:
            return None
        return out

    def _device_probe(self, capacity=0):
        """the probe set of this callback on its device (re-made when more rows are asked for)"""
        fields = self._device_fields()
        dev = fields[0][0].device
        if self._probe is not None and (self._probe[0] is not dev or self._probe[2] < capacity):
            self._probe[0].probe_destroy(self._probe[1])
            self._probe = None
        if self._probe is None:
            loc = self._locate()
            pid = dev.probe_create(loc.cells, loc.weights, [code for _, code in fields], capacity=capacity)
            self._probe = (dev, pid, capacity)
        return self._probe

    def row_probe(self, n_rows):
        """(device, probe id) that can take ``n_rows`` rows after the steps of a batch, or None when this callback cannot be
        sampled that way (a field not on the device, several ranks)"""
        from .pointeval import device_ready
        fields = self._device_fields()
        if self._eval_func is not None or fields is None or not hasattr(fields[0][0].device, 'probe_append'):
            return None
        if not all(device_ready(s) for s in set(s for s, _ in fields)):
            return None
        dev, pid, _ = self._device_probe(capacity=n_rows)
        return dev, pid

    def __call__(self):
        from . import pointeval
        if self._eval_func is not None:
            return self._eval_func()
        loc = self._locate()
        fields = self._device_fields()
        if fields is not None and all(pointeval.device_ready(s) for s in set(s for s, _ in fields)):
            dev, pid, _ = self._device_probe(capacity=self._probe[2] if self._probe else 0)
            return dev.probe_eval(pid)
        cols = []
        for f in self.field_names:
            func = self.solver_obj.fields[f]
            v = pointeval.evaluate(func.cell_node_values(), loc.cells, loc.weights)
            cols.append(v.reshape(len(loc.cells), -1))
        return np.hstack(cols)

    # ---- evaluation and the file
    def take_row(self, t, values):
        """one evaluation at time ``t`` with ``values`` already computed (a row of a batch, FlowSolver2d.create_iterator)"""
        if t < self.start_time or t > self.end_time:
            return
        self.history.append((t, np.asarray(values)))
        if self.append_to_log:
            self.push_to_log(t, values)

    def evaluate(self, index=None):
        t = self.solver_obj.simulation_time
        if t < self.start_time or t > self.end_time:
            return
        self.take_row(t, self())

    def export(self):
        """rank 0 rewrites diagnostic_<name>.npz with the history so far"""
        if not self.export_to_hdf5 or getattr(self.solver_obj.comm, 'rank', 0) != 0:
            return
        outdir = self.outputdir or self.solver_obj.options.output_directory
        os.makedirs(outdir, exist_ok=True)
        n, width = len(self.history), sum(self.field_dims)
        data = {'time': np.array([h[0] for h in self.history], dtype=np.float64).reshape(n, 1)}
        rows = np.array([h[1] for h in self.history], dtype=np.float64).reshape(n, len(self.detector_names), width)
        for i, dn in enumerate(self.detector_names):
            data[dn] = rows[:, i, :]
        data['field_names'] = np.array(self.field_names)
        data['field_dims'] = np.array(self.field_dims)
        data['detector_names'] = np.array(self.detector_names)
        data['detector_xy'] = np.array(self.detector_locations, dtype=np.float64).reshape(-1, 2)
        path = os.path.join(outdir, 'diagnostic_{:}.npz'.format(self.name))
        tmp = path + '.tmp.npz'
        np.savez(tmp, **data)
        os.replace(tmp, path)


def TimeSeriesCallback2D(solver_obj, fieldnames, x, y, location_name, z=None, outputdir=None, export_to_hdf5=True,
                         append_to_log=True, eval_func=None, start_time=None, end_time=None, tolerance=1e-3):
    """Time series of fields at one point (thetis/callback.py:629-749), named ``timeseries_<location>_<fields>``: a detector set of
    one point.  ``eval_func(field, (x, y))``, if given, replaces the point evaluation (host; such a callback is not batched)."""
    name = 'timeseries_{:}_{:}'.format(location_name, '-'.join(fieldnames))
    cb = DetectorsCallback(solver_obj, [(x, y)], fieldnames, name, detector_names=[location_name], outputdir=outputdir,
                           export_to_hdf5=export_to_hdf5, append_to_log=append_to_log, start_time=start_time, end_time=end_time)
    if eval_func is not None:
        def call():
            vals = [np.atleast_1d(np.asarray(eval_func(solver_obj.fields[f], (x, y)), dtype=np.float64)) for f in fieldnames]
            return np.concatenate(vals).reshape(1, -1)
        cb._eval_func = call
    return cb
