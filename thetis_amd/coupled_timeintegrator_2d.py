"""
Coupled 2D time integrator: shallow water step, then every tracer with the UPDATED velocity, then the limiter once per
time step (thetis/coupled_timeintegrator_2d.py:93-113).  All of it stays on the device: the tracers are extra DG-P1
fields of the same C-ABI handle that steps the shallow water equations.
"""
import numpy as np

from . import reactions
from .function import Function
from .log import print_output
from .options import Constant
from .rungekutta import advance_with_rows
from .timeintegrator import TimeIntegratorBase

__all__ = ['DeviceTracerSSPRK33', 'DeviceTracerForwardEuler', 'DeviceSedimentSSPRK33', 'DeviceSedimentForwardEuler',
           'GeneralCoupledTimeIntegrator2D']


def _velocity_factor(f):
    """options.tracer_advective_velocity_factor: a Constant, or a Function that is spatially constant (as in
    test/tracerEq/test_h-advection_mes_2d.py:52-53); a varying Function is not on the device path."""
    if isinstance(f, Function):
        d = f.dat.data_ro
        if d.size and np.abs(d - d.flat[0]).max() > 1e-14*max(1.0, abs(float(d.flat[0]))):
            raise NotImplementedError('a spatially varying tracer_advective_velocity_factor is not on the device path')
        return float(d.flat[0]) if d.size else 1.0
    return float(f)


class _AttrDict(dict):
    def __init__(self, *args, **kwargs):
        super(_AttrDict, self).__init__(*args, **kwargs)
        self.__dict__ = self


def _cval(v):
    return None if v is None else float(v)


def _vec(v):
    """constant 2-vector given as a tuple / array / vector Constant"""
    a = np.asarray(v.values() if hasattr(v, 'values') and callable(v.values) else v, dtype=float).ravel()
    assert a.shape == (2,), "tracer boundary 'uv' must be a constant 2-vector"
    return a


class DeviceTracerSSPRK33(object):
    """SSPRK33 of one tracer equation on the device handle of the shallow water stepper (rungekutta.py:870-952)."""
    n_stages = 3
    c = (0.0, 1.0, 0.5)

    def __init__(self, equation, solution, fields, dt, options, bnd_conditions, swe_stepper):
        equation.check_bnd_conditions(bnd_conditions)
        self.equation, self.solution, self.fields, self.dt = equation, solution, fields, dt
        self.bnd_conditions = bnd_conditions or {}
        self.swe = swe_stepper
        self.device = swe_stepper.device
        self.tid = self.device.add_tracer()
        self._uploaded = None
        self._device_ahead = False
        self.solution._pull_hook = self._pull
        self.solution._device_field = (self, self.tid)
        self._src_signature = None
        # a source that is an expression of tracer Functions (thetis_amd/reactions.py) is evaluated on the device in front of every
        # stage.  The tracer steppers are created one after another, so whether a Function operand is a tracer is only known when
        # the coupled integrator has them all: resolve_reaction, called from there.
        self._reaction = None
        self._host_reaction = None
        self._reaction_pending = reactions.has_function_leaf(fields.get('source-{:}'.format(equation.label)))
        if not self._reaction_pending:
            self._push_source()
        if getattr(equation, 'conservative', False):
            self.device.tracer_set_conservative(self.tid, True)
        mu = fields.get('diffusivity_h-{:}'.format(equation.label))
        self.diffusive = mu is not None
        if self.diffusive:                      # HorizontalDiffusionTerm, tracer_eq_2d.py:226-278
            self.device.tracer_set_diffusivity(self.tid, swe_stepper._vertex_coefficient(mu),
                                               float(equation.options.sipg_factor_tracer))
        self._push_bcs()

    def _tracer_of(self, f):
        """tracer id of a Function that is the solution of a tracer on this device; < 0: a field of the flow; None: neither"""
        df = getattr(f, '_device_field', None)
        if df is None or getattr(df[0], 'device', None) is not self.device:
            return None
        if isinstance(df[1], str):              # 'uv' / 'elev' of the shallow water stepper (rungekutta.py)
            return -1
        return int(df[1])

    def resolve_reaction(self):
        """decide, now that every tracer stepper exists, whether the source reacts; compile it if so"""
        if not self._reaction_pending:
            return
        self._reaction_pending = False
        src = self.fields.get('source-{:}'.format(self.equation.label))
        if not reactions.is_reactive(src, self._tracer_of):     # (a flow operand counts: compile_source refuses it by name)
            self._push_source()                 # today's path: nodal values, once
            return
        mesh = self.equation.mesh
        comm = getattr(self.swe, 'comm', None)
        if comm is not None and comm.size > 1:
            raise NotImplementedError('a tracer source that depends on tracers is not available on several ranks (the partitioned '
                                      'stepper carries no reaction programs)')
        npc = int(np.asarray(mesh.cells).shape[1])
        if npc == 4 and not getattr(mesh, 'affine', True):
            raise NotImplementedError('a tracer source that depends on tracers needs triangles or parallelograms: on a non-affine '
                                      'quadrilateral mesh the Jacobian varies inside a cell')
        shared = self.device.__dict__.setdefault('_reaction_fields', [])
        self._reaction = reactions.compile_source(src, self._tracer_of, npc, shared)
        shared[:] = self._reaction.fields
        self._reaction_set = False
        if not hasattr(self.device, 'tracer_set_reaction'):
            if not hasattr(self.device, 'tracer_get_buffer'):
                raise NotImplementedError('a device class without tracer_set_reaction must give the stage buffers of a tracer '
                                          '(tracer_get_buffer) for the host evaluation of a reacting source')
            self._host_reaction = reactions.HostReaction(self._reaction, mesh.cell_xy())
        self._push_source()

    def _host_source(self, i_in):
        """host fallback: the source of the stage that reads buffer ``i_in``, from the tracers as they are on the device"""
        vals = {j: self.device.tracer_get_buffer(j, i_in if j == self.tid else 0) for j in self._reaction.tracers}
        self.device.tracer_set_source(self.tid, self._host_reaction.evaluate(vals))

    def _push_source(self):
        """(re-)upload the tracer source when it changed (a Function updated by update_forcings, or a Constant)"""
        if self._reaction_pending:
            return
        if self._reaction is not None:
            p = self._reaction
            if self._host_reaction is not None:
                return                          # evaluated per stage from the live Constants and Functions (_host_source)
            sig = p.signature()
            if sig != self._src_signature:
                seen = self.device.__dict__.setdefault('_reaction_field_versions', {})
                for slot, f in enumerate(p.fields):
                    if seen.get(slot) != (id(f), f._host_version):
                        self.device.reaction_set_field(slot, f.cell_node_values())
                        seen[slot] = (id(f), f._host_version)
                if not self._reaction_set:
                    self.device.tracer_set_reaction(self.tid, p.code, p.constant_values(), p.phi, p.w)
                    self._reaction_set = True
                else:
                    self.device.tracer_set_reaction_constants(self.tid, p.constant_values())
                self._src_signature = sig
            return
        src = self.fields.get('source-{:}'.format(self.equation.label))
        sig = self.swe._signature(src)
        if sig != self._src_signature:
            self.device.tracer_set_source(self.tid, None if src is None else self.swe._nodal(src))
            self._src_signature = sig

    def _push_bcs(self):
        for marker in self.equation.mesh.boundary_markers:
            funcs = self.bnd_conditions.get(marker)
            v = None if funcs is None else funcs.get('value')
            is_field = isinstance(v, Function)
            sig = None if funcs is None else tuple(sorted((k, self.swe._signature(x)) for k, x in funcs.items()))
            cache = self.__dict__.setdefault('_bc_signatures', {})
            if marker in cache and cache[marker] == sig:
                continue                # nothing on this marker changed since the last upload
            cache[marker] = sig
            if is_field:            # Function-valued 'value': the nodal values of the boundary cells only (compact upload)
                mesh = self.equation.mesh
                cells, _ = self.device.boundary_facets(self.device._slot(marker))
                fs = v.function_space()
                if fs.family == 'CG':
                    vals = v.dat.data_ro[np.asarray(mesh.cells)[cells]]
                else:
                    vals = v.cell_node_values()[cells]
                self.device.tracer_set_bc_facets(self.tid, self.device._slot(marker), vals)
            else:
                self.device.tracer_set_bc(self.tid, marker, _cval(v))
            uv_b = None if funcs is None else funcs.get('uv')
            un_b = None if funcs is None else funcs.get('un')
            fl_b = None if funcs is None else funcs.get('flux')
            el_b = None if funcs is None else funcs.get('elev')
            def entry(x, vector=False):
                """a Constant / number, or a Function as the values at the end nodes of the marker's boundary facets"""
                if x is None:
                    return None
                if isinstance(x, Function):
                    fs = x.function_space()
                    if fs.family == 'CG':
                        return self.device.facet_node_values(marker, x.dat.data_ro, cells_of_vertices=self.equation.mesh.cells)
                    return self.device.facet_node_values(marker, x.cell_node_values())
                return _vec(x) if vector else _cval(x)
            self.device.tracer_set_bc_velocity(self.tid, marker, uv=entry(uv_b, vector=True), un=entry(un_b), flux=entry(fl_b),
                                               elev=None if el_b is None else _cval(el_b))
            if self.diffusive:                  # boundary term of the diffusion operator, tracer_eq_2d.py:264-277
                if funcs is None:
                    kind, dfl = 0, 0.0
                elif 'diff_flux' in funcs:
                    kind, dfl = 1, _cval(funcs['diff_flux'])
                elif 'value' not in funcs:
                    kind, dfl = 3, 0.0
                else:
                    kind, dfl = (4 if is_field else 2), 0.0
                self.device.tracer_set_diffusion_bc(self.tid, marker, kind, dfl)

    def _before_stage(self, i_in):
        """in front of the stage launch that reads buffer ``i_in`` (the sediment stepper's host fallback writes its source here)"""

    def _pull(self):
        if self._device_ahead:
            self.solution._data[...] = self.device.tracer_get_state(self.tid).reshape(self.solution._data.shape)
            self._device_ahead = False

    def _sync_to_device(self):
        if self._uploaded != self.solution._host_version:
            self._pull()
            self.device.tracer_set_state(self.tid, self.solution._data.reshape(-1, self.device.npc))
            self._uploaded = self.solution._host_version
            self._device_ahead = False

    def initialize(self, solution):
        self._uploaded = None
        self._sync_to_device()

    def set_dt(self, dt):
        self.dt = dt            # the handle's dt is set by the shallow water stepper

    def solve_stage(self, i_stage, t, update_forcings=None):
        if update_forcings is not None:
            update_forcings(t + self.c[i_stage]*self.dt)
            self._push_bcs()
            self._push_source()
        if i_stage == 0:
            self._sync_to_device()
        if self._reaction is not None:
            self._push_source()                 # (a Constant of the source may have changed without update_forcings)
            if self._host_reaction is not None:
                self._host_source(i_stage)
        self._before_stage(i_stage)
        self.device.tracer_solve_stage(self.tid, i_stage)
        self._device_ahead = True

    def advance(self, t, update_forcings=None):
        for i in range(self.n_stages):
            self.solve_stage(i, t, update_forcings)


class DeviceTracerForwardEuler(DeviceTracerSSPRK33):
    """timeintegrator.ForwardEuler of one tracer equation (thetis/timeintegrator.py:115-165)."""
    n_stages = 1
    c = (0.0,)

    def solve_stage(self, i_stage, t, update_forcings=None):
        assert i_stage == 0
        self.advance(t, update_forcings)

    def advance(self, t, update_forcings=None):
        if update_forcings is not None:
            update_forcings(t + self.dt)
            self._push_bcs()
            self._push_source()
        self._sync_to_device()
        if self._reaction is not None:
            self._push_source()
            if self._host_reaction is not None:
                self._host_source(0)
        self._before_stage(0)
        self.device.tracer_forward_euler(self.tid)
        self._device_ahead = True


class _SedimentStepper(object):
    """The sediment field as one more device tracer (thetis/sediment_eq_2d.py): its source comes from the sediment model's planes
    in front of every stage (csrc/swe2d_sediment.hip), and a marker with ``'equilibrium'`` takes its outer value from the model."""
    sediment_model = None

    host_sediment = False

    def attach_sediment(self, model):
        """``model`` becomes this tracer's source.  A device class with the sediment calls runs the passes itself; one without
        them gets them from the host replay (``HostSediment``), as the reaction and particle passes do: the source per stage from the
        stage's input buffer, the 'equilibrium' values per step through the per-facet table, the Exner update through
        ``set_bathymetry`` - one transfer of the field per stage and of the flow per step."""
        self.sediment_model = model
        if hasattr(self.device, 'sediment_set'):
            model.bind_device(self.device, self.tid)
        else:
            need = ['tracer_get_buffer', 'tracer_set_bc_facets']
            if self.equation.options.sediment_model_options.solve_exner:
                need.append('set_bathymetry')
            missing = [n for n in need if not hasattr(self.device, n)]
            if missing:
                raise NotImplementedError('sediment_model_options: a device class without the sediment passes must give {:} for the '
                                          'host evaluation'.format(', '.join(missing)))
            self.host_sediment = True
        self._push_bcs()

    def sediment_update(self):
        """the model on the current flow, once per time step; host fallback: the 'equilibrium' facets as well"""
        self.sediment_model.update()
        if self.host_sediment:
            self._push_host_equilibrium()

    def _host_fields(self):
        m = self.sediment_model
        return m.elev.cell_node_values(), m._bathymetry()

    def _push_host_equilibrium(self):
        m = self.sediment_model
        if m._planes is None:
            return
        eta, bath = self._host_fields()
        vals = m.host.boundary_values(m._planes[2], eta, bath)
        for marker in self.equation.mesh.boundary_markers:
            if 'equilibrium' in (self.bnd_conditions.get(marker) or {}):
                slot = self.device._slot(marker)
                cells, _ = self.device.boundary_facets(slot)
                self.device.tracer_set_bc_facets(self.tid, slot, vals[cells])
                if self.diffusive:
                    self.device.tracer_set_diffusion_bc(self.tid, marker, 4, 0.0)

    def _before_stage(self, i_in):
        if not self.host_sediment:
            return
        m = self.sediment_model
        E, D, _ = m._terms()
        eta, bath = self._host_fields()
        self.device.tracer_set_source(self.tid, m.host.source(E, D, self.device.tracer_get_buffer(self.tid, i_in), eta, bath))

    def exner_step(self, solver):
        """the bed update after the sediment step (and limiter), the bedload pass on the new flow in front of it"""
        m = self.sediment_model
        contrib = m.update_bedload() if m.use_bedload else None
        slide = m.update_slide(self.dt) if m.use_sediment_slide else None
        if not self.host_sediment:
            self.device.exner_step()
            return
        E, D, _ = m._terms()
        eta, bath = self._host_fields()
        new = m.host.exner(E, D, self.device.tracer_get_state(self.tid), eta, bath, self.dt, bedload=contrib, slide=slide)
        self.device.set_bathymetry(new)
        b = solver.fields.bathymetry_2d
        b._data[...] = new.reshape(b._data.shape)
        b._host_version += 1

    def _push_bcs(self):
        full = self.bnd_conditions
        self.bnd_conditions = {m: (None if f is None else {k: v for k, v in f.items() if k != 'equilibrium'}) for m, f in full.items()}
        try:
            super(_SedimentStepper, self)._push_bcs()
        finally:
            self.bnd_conditions = full
        if self.sediment_model is None:
            return
        if self.host_sediment:
            self._push_host_equilibrium()
            return
        for marker in self.equation.mesh.boundary_markers:
            eq = 'equilibrium' in (full.get(marker) or {})
            self.device.sediment_set_equilibrium_bc(marker, eq)
            if eq and self.diffusive:           # the diffusion operator's boundary term reads the same per-facet table
                self.device.tracer_set_diffusion_bc(self.tid, marker, 4, 0.0)


class DeviceSedimentSSPRK33(_SedimentStepper, DeviceTracerSSPRK33):
    pass


class DeviceSedimentForwardEuler(_SedimentStepper, DeviceTracerForwardEuler):
    pass


class BedloadStepper(object):
    """The bed of a run with ``use_bedload`` and / or ``use_sediment_slide`` and no sediment field (the reference's meander and its
    slide test): after the flow step (and the tracers) the bedload pass, the slide pass and the Exner update, on the device where
    it has the calls, through ``HostSediment`` and ``set_bathymetry`` otherwise."""

    def __init__(self, model, device, dt):
        self.sediment_model, self.device, self.dt = model, device, dt
        need = (['bedload_set'] if model.use_bedload else []) + (['slide_set'] if model.use_sediment_slide else [])
        self.host_sediment = not all(hasattr(device, n) for n in need)
        if not self.host_sediment:
            model.bind_bedload_device(device)
        elif not hasattr(device, 'set_bathymetry'):
            raise NotImplementedError('sediment_model_options: a device class without the bedload and slide passes must give '
                                      'set_bathymetry for the host evaluation')

    def set_dt(self, dt):
        self.dt = dt

    def exner_step(self, solver):
        m = self.sediment_model
        contrib = m.update_bedload() if m.use_bedload else None
        slide = m.update_slide(self.dt) if m.use_sediment_slide else None
        if not self.host_sediment:
            self.device.exner_step()
            return
        new = m.host.exner(None, None, None, m.elev.cell_node_values(), m._bathymetry(), self.dt, bedload=contrib, slide=slide)
        self.device.set_bathymetry(new)
        b = solver.fields.bathymetry_2d
        b._data[...] = new.reshape(b._data.shape)
        b._host_version += 1


class GeneralCoupledTimeIntegrator2D(TimeIntegratorBase):
    def __init__(self, solver, swe_stepper, tracer_steppers, bed=None):
        self.bed = bed                          # a BedloadStepper: the bed of a run without a sediment field
        self.solver = solver
        self.options = solver.options
        self.fields = solver.fields
        self.timesteppers = _AttrDict(swe2d=swe_stepper)      # AttrDict in the reference (coupled_timeintegrator_2d.py:33)
        self.timesteppers.update(tracer_steppers)
        self.swe = swe_stepper
        self.tracers = tracer_steppers
        self.device = swe_stepper.device
        print_output('Coupled time integrator: {:}'.format(self.__class__.__name__))
        if not self.options.tracer_only:
            print_output('  Shallow Water time integrator: {:}'.format(swe_stepper.__class__.__name__))
        print_output('  Tracer time integrator: {:}'.format(self.options.tracer_timestepper_type))
        o = self.options
        self.device.tracer_set_options(o.use_lax_friedrichs_tracer, float(o.lax_friedrichs_tracer_scaling_factor),
                                       _velocity_factor(o.tracer_advective_velocity_factor))
        for ts in tracer_steppers.values():     # every tracer has its id now: which sources react (thetis_amd/reactions.py)
            ts.resolve_reaction()
        self.reacting = [ts for ts in tracer_steppers.values() if ts._reaction is not None]
        self.host_reactions = any(ts._host_reaction is not None for ts in self.reacting)
        # (a sediment field the HOST evaluates needs the stage buffers as well: stage by stage)
        self.host_reactions = self.host_reactions or any(getattr(ts, 'host_sediment', False) for ts in tracer_steppers.values())
        self.host_reactions = self.host_reactions or (bed is not None and bed.host_sediment)

    def set_dt(self, dt):
        for stepper in sorted(self.timesteppers):
            self.timesteppers[stepper].set_dt(dt)
        if self.bed is not None:
            self.bed.set_dt(dt)

    def initialize(self, solution2d):
        assert solution2d == self.fields.solution_2d
        self.swe.initialize(self.fields.solution_2d)
        for label, ts in self.tracers.items():
            ts.initialize(self.fields[label])

    def advance(self, t, update_forcings=None):
        """coupled_timeintegrator_2d.py:93-113"""
        use_limiter = self.options.use_limiter_for_tracers and self.options.polynomial_degree > 0
        # (a reacting source the HOST evaluates needs the tracers between the stages: stage by stage)
        fused = all(ts.n_stages == 3 for ts in self.tracers.values()) and self.swe.n_stages == 3 and not self.host_reactions
        if update_forcings is None and fused and not self.swe.forced_per_stage:        # all SSPRK33: one C call per time step
            self.swe._sync_to_device()
            for ts in self.tracers.values():
                ts._sync_to_device()
                if getattr(ts, 'sediment_model', None) is not None:
                    ts.sediment_model._planes = None      # (the batch refreshes the planes on the device)
            for ts in self.reacting:
                ts._push_source()               # (a changed Constant of a program)
            self.swe._tide_clock(t)
            self.device.advance_coupled(1, tracer_only=self.options.tracer_only, use_limiter=use_limiter)
            self.swe._device_ahead = True
            for ts in self.tracers.values():
                ts._device_ahead = True
            self._bed_moved()
            return
        if not self.options.tracer_only:
            self.swe.advance(t, update_forcings=update_forcings)
        else:
            self.swe._sync_to_device()
        if self.reacting:                       # a reacting source reads the OTHER tracers on the device
            for ts in self.tracers.values():
                ts._sync_to_device()
        for label, ts in self.tracers.items():
            # the sediment field comes last (coupled_timeintegrator_2d.py:100-135): the model on the new flow, its coefficients
            # frozen over the step, the sediment stages, the limiter, the Exner update
            sed = getattr(ts, 'sediment_model', None)
            if sed is not None:
                ts._sync_to_device()
                ts.sediment_update()
            ts.advance(t, update_forcings=update_forcings)
            if use_limiter:
                self.device.tracer_limit(ts.tid)
            if sed is not None and self.options.sediment_model_options.solve_exner:
                ts.exner_step(self.solver)
                self._bed_moved()
        if self.bed is not None:                # no sediment field: the bedload pass on the new flow, then the bed
            self.bed.exner_step(self.solver)
            self._bed_moved()

    @property
    def forced_per_stage(self):
        return self.swe.forced_per_stage

    @property
    def wants_clock(self):
        return self.swe.wants_clock

    def advance_steps(self, t, n_steps, probes=None, clock=None):
        """``n_steps`` coupled steps without forcing updates; one library call when every stepper is SSPRK33.  ``probes``: probe
        sets of the device that take one row after every step (FlowSolver2d.create_iterator).  ``clock`` = (t_start, n_done) of
        the time loop, for a tide the device evaluates (SSPRK33.advance_steps)."""
        use_limiter = self.options.use_limiter_for_tracers and self.options.polynomial_degree > 0
        fused = all(ts.n_stages == 3 for ts in self.tracers.values()) and self.swe.n_stages == 3 and not self.host_reactions
        if not fused:
            done = [0]

            def one_by_one(j):
                for _ in range(j):
                    i = done[0]
                    self.advance(t + i*self.swe.dt if clock is None else clock[0] + (clock[1] + i)*self.swe.dt)
                    done[0] += 1
            advance_with_rows(self.device, n_steps, one_by_one, probes or (), self.swe._step_end_time(t, clock))
            return
        self.swe._sync_to_device()
        for ts in self.tracers.values():
            ts._sync_to_device()
        self.swe._tide_clock(*(clock if clock is not None else (t, 0)))
        for ts in self.reacting:
            ts._push_source()
        if probes:
            advance_with_rows(self.device, n_steps,
                              lambda j: self.device.advance_coupled(j, tracer_only=self.options.tracer_only, use_limiter=use_limiter),
                              probes, self.swe._step_end_time(t, clock))
        else:
            self.device.advance_coupled(int(n_steps), tracer_only=self.options.tracer_only, use_limiter=use_limiter)
        self.swe._device_ahead = True
        for ts in self.tracers.values():
            ts._device_ahead = True
        self._bed_moved()

    def _bed_moved(self):
        """after a step with solve_exner the host copy of fields.bathymetry_2d is stale (read back on demand, solver2d.py)"""
        if self.options.sediment_model_options.solve_exner:
            host = any(getattr(ts, 'host_sediment', False) for ts in self.tracers.values())
            host = host or (self.bed is not None and self.bed.host_sediment)
            if self.bed is not None:
                self.bed.sediment_model._qb = None
                if self.bed.sediment_model.on_device:
                    self.bed.sediment_model._slide = None
            self.solver._bed_device_ahead = not host            # (the host fallback wrote fields.bathymetry_2d itself)
            for ts in self.tracers.values():
                if getattr(ts, 'sediment_model', None) is not None:
                    ts.sediment_model._planes = None
                    ts.sediment_model._qb = None
                    if ts.sediment_model.on_device:
                        ts.sediment_model._slide = None

    def diagnostics(self):
        return self.swe.diagnostics()
