#!/usr/bin/env python
"""Range-check pass over the kernels (tools/range_check.sh): exercises every kernel family of the library on small meshes
against the -DSWE_RANGE_CHECK build, in which every raw-buffer access of the stage / tracer / viscosity / diagnostics kernels
is tested against the table of the library's own allocations (swe2d_kernels.h).  Prints the report and exits non-zero on a
violation.  THETIS_AMD_RANGE_SELFTEST=1 (negative control): the table records HALF of every allocation - violations expected.
(The image has no AddressSanitizer-enabled HIP runtime: an ASAN build of the library compiles for gfx950:xnack+ but cannot
be loaded, so this is the sanitizer pass of SURVEY.md section 5 for the device code.)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def exercise(only=None):
    from helpers import channel_case, delaunay_case, quad_case
    from thetis_amd import _lib, ordering
    from thetis_amd.device import Swe2dDevice
    n_launch = 0
    for name, case in (('triangles', channel_case(nx=23, ny=11, seed=1)), ('quadrilaterals', quad_case(nx=17, ny=9, seed=2)),
                       ('unstructured', delaunay_case(n_points=500, seed=3)[:4])):
        mesh, bath, uv, eta = case
        k = mesh.cells.shape[1]
        cxy = mesh.cell_xy()
        for variant in ('plain', 'open+fields', 'sources', 'viscosity', 'wetting-drying', 'tracers', 'farms', 'farms+wetting-drying', 'dfarm', 'tide', 'atm', 'stats',
                        'stats+wetting-drying', 'particles', 'particles+wetting-drying', 'reactions', 'sediment', 'sections'):
            if only and variant not in only:
                continue
            # (farms: deep water, so that the radicand of the upwind correction stays positive)
            bath_v = bath - 0.6*bath.max() if variant.endswith('wetting-drying') and not variant.startswith('farms') else (bath + 20.0 if variant.startswith('farms') or variant == 'dfarm' else bath)
            dev = Swe2dDevice(mesh, bath_v, 0.05, boundary_len=mesh.boundary_len)
            markers = mesh.boundary_markers
            if variant == 'open+fields':
                dev.set_bc(markers[0], {'elev': 0.2*np.sin(cxy[:, :, 1]/3e3)})
                dev.set_bc(markers[-1], {'un': 0.05, 'drag': 0.01})
            if variant == 'sources':
                dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
                dev.set_field(_lib.FIELD_CORIOLIS, 1e-4*np.ones((mesh.num_cells, k)))
                dev.set_field(_lib.FIELD_WIND_STRESS, 0.1*np.ones((mesh.num_cells, k, 2)))
            if variant == 'viscosity':
                dev.set_viscosity(20.0 + 5.0*np.arange(mesh.num_vertices)/mesh.num_vertices, use_grad_div_viscosity_term=True)
                dev.set_bc(markers[0], {'un': 0.1})
            if variant in ('wetting-drying', 'stats+wetting-drying', 'particles+wetting-drying'):
                dev.set_wetting_and_drying(0.5)
                dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
            if variant.startswith('farms'):
                # tidal turbine farms: the density planes and the farm-cell list are read through the checked loads (stage kernels and
                # swe_turbine_power_kernel); the farms' constant table is read through plain pointers and the power rows are written
                # with atomics - those accesses are not seen by the check (host-checked sizes: one SweFarmTable, capacity + 1 rows)
                if variant == 'farms':
                    dev.set_scalar(_lib.SCALAR_QUADRATIC_DRAG, 0.0025)
                else:
                    dev.set_wetting_and_drying(0.5)
                    dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
                xc = cxy[:, :, 0].mean(axis=1)
                half = xc > np.median(xc)
                par = _lib.TurbineParams()
                par.rotor_area, par.projected_diameter, par.rho0, par.upwind_correction = 254.0, 18.0, 1000.0, 1
                par.n_table = 5
                for j, (sp, ct) in enumerate(zip([0.01, 0.02, 0.05, 0.08, 0.1], [0.01, 0.7, 0.7, 0.1, 0.0001])):
                    par.speeds[j], par.thrust[j], par.power[j] = sp, ct, 0.5*ct
                dev.turbine_farm_set(0, par, np.where(half[:, None], 2e-5, 0.0)*np.ones((mesh.num_cells, k)))
                par2 = _lib.TurbineParams()
                par2.rotor_area, par2.projected_diameter, par2.rho0 = 254.0, 18.0, 1000.0
                par2.thrust_area_const, par2.power_const, par2.support_area = 0.8*254.0, 0.4, 5.0
                dens = 1e-5*np.ones((mesh.num_cells, k))
                dens[-1] = 0.0                       # ... whose farm-cell list ends one short of the last cell
                dev.turbine_farm_set(3, par2, dens)
                assert dev.flow_supported() == 0 and not dev.fused_pair_info()[0]
            if variant == 'dfarm':
                # discrete turbine farms (csrc/swe2d_dfarm.hip): the cell list, the CSR of candidate turbines and its transpose, the
                # coordinates, the density table, the state planes and the mesh arrays are read and the output velocity is written
                # through the checked accesses - by the density kernel at set-up, the drag pass after every stage launch of the
                # advances below, the power pass and the per-turbine pass (rule and constants: kernel arguments / the SweFarmTable;
                # limb sums: atomics on host-checked sizes).  One farm over the whole mesh with overlapping turbines, one outside
                # and one clipped by the boundary; a second on half of the cells with the largest rule.
                from thetis_amd.function import farm_quadrature
                lo, hi = cxy.reshape(-1, 2).min(axis=0), cxy.reshape(-1, 2).max(axis=0)
                span = hi - lo
                par = _lib.TurbineParams()
                par.rotor_area, par.projected_diameter, par.rho0, par.upwind_correction = 254.0, 0.3*span[1], 1000.0, 1
                par.thrust_area_const, par.power_const, par.support_area = 0.8*254.0, 0.4, 5.0
                txy = lo + span*np.array([[0.3, 0.4], [0.35, 0.5], [0.7, 0.02], [1.0, 1.0], [2.0, 0.5]])
                dev.dfarm_set(1, par, txy, np.ones(mesh.num_cells, dtype=bool), *farm_quadrature(k, 10))
                half = cxy[:, :, 0].mean(axis=1) > np.median(cxy[:, :, 0].mean(axis=1))
                dev.dfarm_set(6, par, txy[:2] + 0.3*span*np.array([1.0, 0.0]), half, *farm_quadrature(k, 14))
                assert len(dev.dfarm_density_read(1)[0]) > 0 and len(dev.dfarm_density_read(6)[0]) > 0
                assert dev.flow_supported() == 0 and not dev.fused_pair_info()[0]
            if variant == 'tide':
                # harmonic tidal boundary elevation: swe_tide_kernel reads its table and the facet list and writes the elevation planes
                # of the boundary fields through the checked accesses, one launch in front of every stage launch of the advances below
                # (the frequencies are kernel arguments)
                from thetis_amd.device import TideValues
                slot = dev._slot(markers[0])
                nf, kc = len(dev.boundary_facets(slot)[0]), 5
                rng = np.random.default_rng(7)
                dev.tide_set([slot], 1.4e-4*(1.0 + np.arange(kc)), 0.1*rng.normal(size=(nf, 2)), 0.2*rng.uniform(size=(kc, nf, 2)),
                             rng.uniform(0.0, 6.0, size=(kc, nf, 2)))
                dev.set_bc(markers[0], {'elev': TideValues()})
                dev.tide_clock(1000.0, 7)
                dev.tide_eval(44714.1)
                assert dev.tide_read().shape == (nf, 2) and np.isfinite(dev.tide_read()).all()
                assert dev.flow_supported() == 0 and not dev.fused_pair_info()[0]
                n_launch += 12
            if variant == 'atm':
                # atmospheric record: swe_atm_kernel reads cv and two snapshots of the record and writes the wind-stress and pressure
                # planes of every cell through the checked accesses, one launch in front of every stage launch of the advances below.
                # A record with one quantity alone (1 and 2 doubles per vertex), then with wind and pressure (3), each evaluated
                # at the first, an interior and the last snapshot time.
                rng = np.random.default_rng(8)
                tm = np.array([0.0, 0.4, 1.7, 2.0, 6.5])
                wu, wv = 30.0*rng.normal(size=(2, len(tm), mesh.num_vertices))
                pa = 101325.0 + 500.0*rng.normal(size=(len(tm), mesh.num_vertices))
                for tabs in ((None, None, pa), (wu, wv, None), (wu, wv, pa)):
                    dev.atm_set(tm, *tabs)
                    for t_eval in (tm[0], tm[2], tm[-1]):
                        dev.atm_eval(t_eval)
                    w_read, p_read = dev.atm_read(wind=tabs[0] is not None, pressure=tabs[2] is not None)
                    assert all(a is None or np.isfinite(a).all() for a in (w_read, p_read))
                    n_launch += 3
                dev.tide_clock(0.0, 2)
                assert dev.flow_supported() == 0 and not dev.fused_pair_info()[0]
                n_launch += 12
            dev.set_state(0.1*uv, 0.1*np.abs(eta))
            if variant.startswith('farms'):
                dev.turbine_rows_reserve(3)
                for _ in range(3):
                    dev.advance(1)
                    dev.turbine_rows_append()
                rows = dev.turbine_rows_read()
                assert rows.shape[0] == 3 and np.isfinite(rows).all() and (rows[:, [0, 3]] >= 0).all() and rows[:, 3].min() > 0, rows
                assert np.isfinite(dev.turbine_power()).all()
                n_launch += 8
            if variant == 'dfarm':
                dev.turbine_rows_reserve(2)
                for _ in range(2):
                    dev.advance(1)
                    dev.turbine_rows_append()
                rows = dev.turbine_rows_read()
                each = dev.dfarm_turbine_power(1)
                assert rows.shape[0] == 2 and np.isfinite(rows).all() and rows[:, 1].min() > 0 and rows[:, 6].min() > 0, rows
                assert each.shape == (5,) and np.isfinite(each).all() and each[4] == 0.0 and each[:2].min() > 0, each
                n_launch += 12
            if variant.startswith('stats'):
                # running field statistics: swe_stats_kernel reads the state planes (wetting-drying: also the cell vertices, alpha and the
                # bathymetry) and read-modify-writes the accumulator planes of its set through the checked accesses; the weights are
                # kernel arguments.  (swe_stats_fill_kernel writes through a plain pointer: host-checked size, the whole allocation.)
                sets = {kc: dev.stats_create(kc) for kc in (0, 5, 32)}
                for j in range(3):
                    dev.advance(1)
                    for kc, sid in sets.items():
                        arg = 1.4e-4*(1.0 + np.arange(kc))*(44714.1 + 300.0*j)
                        dev.stats_append(sid, np.stack([np.cos(arg), np.sin(arg)], axis=1).reshape(-1) if kc else None)
                for kc, sid in sets.items():
                    acc, n = dev.stats_read(sid)
                    assert n == 3 and acc.shape == (8 + 2*kc, mesh.num_cells, k) and np.isfinite(acc).all(), (name, variant, kc)
                    assert (acc[0] <= acc[1]).all() and (acc[2] >= 0).all()
                dev.stats_destroy(sets[5])
                n_launch += 12
            if variant.startswith('particles'):
                # Lagrangian particles: swe_particle_kernel reads the cell vertices, the vertex coordinates, the neighbour codes and the
                # velocity planes of every cell a walk visits and reads / writes the position and the four int planes of its set
                # through the checked accesses (the rows are copied by the runtime).  Short moves, moves across many cells that end at
                # walls and open boundaries, and moves that reach the hop cap; one particle, a partial and several workgroups.
                # Quadrilaterals: the set is refused.
                rng = np.random.default_rng(9)
                if k != 3:
                    try:
                        dev.particles_create(cxy[:1].mean(axis=1), [0])
                        raise AssertionError('a particle set on quadrilaterals')
                    except _lib.Swe2dError as e:
                        assert e.code == _lib.ERR_UNSUPPORTED
                else:
                    span = np.ptp(cxy.reshape(-1, 2), axis=0).max()
                    sets = []
                    for n_p in (1, 200, 700):
                        pc = rng.integers(0, mesh.num_cells, size=n_p)
                        w = rng.uniform(0.05, 1.0, size=(n_p, 3))
                        w /= w.sum(axis=1, keepdims=True)
                        sets.append(dev.particles_create((w[:, :, None]*cxy[pc]).sum(axis=1), pc, capacity=4))
                    for dt_move in (0.01*span, 2.0*span, 200.0*span):       # |u| ~ 0.05: a fraction of a cell ... past the hop cap
                        dev.advance(1)
                        for pid in sets:
                            dev.particles_advance(pid, dt_move, markers[:1])
                            dev.particles_record(pid)
                    for pid in sets:
                        xy_p, cells_p, status_p, _, _ = dev.particles_read(pid)
                        assert np.isfinite(xy_p).all() and cells_p.min() >= 0 and cells_p.max() < mesh.num_cells, (name, variant)
                        assert dev.particles_read_rows(pid).shape[0] == 3
                    assert (dev.particles_read(sets[2])[2] != 0).any(), (name, variant)
                    dev.particles_destroy(sets[1])
                    n_launch += 9
            if variant == 'tracers':
                tid = dev.add_tracer()
                dev.tracer_set_state(tid, 1.0 + 0.1*np.random.default_rng(0).normal(size=(mesh.num_cells, k)))
                dev.tracer_set_diffusivity(tid, 5.0)
                dev.tracer_set_bc(tid, markers[0], 1.5)
                dev.tracer_set_bc_velocity(tid, markers[0], un=0.1*np.ones((mesh.num_cells, k)))
                dev.advance_coupled(2)
                dev.tracer_diagnostics(tid)
                n_launch += 20
            if variant == 'reactions':
                # reacting tracers: swe_reaction_kernel reads the nodal planes of every tracer and coefficient field its program names
                # and, for X / Y, the cell vertices and vertex coordinates, and writes the source planes of its tracer through the
                # checked accesses, one launch in front of every tracer stage launch below (program, constants and rule: kernel
                # arguments / a buffer the runtime copies).  Gray-Scott with its 9-point rule, then a program with coordinates and
                # two coefficient fields under the 64-point rule; whole-mesh stages, ragged sub-ranges, ForwardEuler and the batch.
                # General quadrilaterals: the program is refused.
                from thetis_amd import Constant, Function, SpatialCoordinate, get_functionspace, reactions
                from thetis_amd.function import farm_quadrature
                P1, P1DG = get_functionspace(mesh, 'CG', 1), get_functionspace(mesh, 'DG', 1)
                fa, fb, fc, fd = Function(P1DG), Function(P1DG), Function(P1), Function(P1DG)
                rng = np.random.default_rng(10)
                for f in (fc, fd):
                    f.assign(rng.uniform(0.5, 1.5, size=f.dat.data_ro.shape))
                for t in range(2):
                    assert dev.add_tracer() == t
                    dev.tracer_set_state(t, rng.uniform(0.2, 1.0, size=(mesh.num_cells, k)))
                tracer_of = lambda f: 0 if f is fa else (1 if f is fb else None)   # noqa: E731
                g, kap = Constant(0.024), Constant(0.06)
                xs, ys = SpatialCoordinate(mesh)
                span = float(np.abs(cxy).max())
                pairs = [(g - fa*fb**2 - g*fa, fa*fb**2 - (g + kap)*fb),
                         (0.01*fc*fa*xs/span - 0.01*fd*fb, 0.01*fd*fb*ys/span - 0.01*fc*fa)]
                if k == 4 and not getattr(mesh, 'affine', True):
                    try:
                        dev.tracer_set_reaction(0, [1], [], *farm_quadrature(4, 2))     # (TRACER 0)
                        raise AssertionError('a reaction program on general quadrilaterals')
                    except _lib.Swe2dError as e:
                        assert e.code == _lib.ERR_UNSUPPORTED
                else:
                    third = mesh.num_cells//3 + 1
                    for j, pair in enumerate(pairs):
                        shared = []
                        for t, src in enumerate(pair):
                            p = reactions.compile_source(src, tracer_of, k, shared)
                            shared[:] = p.fields
                            if j == 1:
                                p.phi, p.w = farm_quadrature(k, 14)
                            for slot, f in enumerate(p.fields):
                                dev.reaction_set_field(slot, f.cell_node_values())
                            dev.tracer_set_reaction(t, p.code, p.constant_values(), p.phi, p.w)
                        for t in range(2):
                            for i in range(3):
                                dev.tracer_solve_stage(t, i)
                            for i in range(3):
                                dev.tracer_solve_stage_cells(t, i, 0, third)
                                dev.tracer_solve_stage_cells(t, i, third, mesh.num_cells)
                            dev.tracer_forward_euler(t)
                            assert np.isfinite(dev.tracer_get_source(t)).all() and np.abs(dev.tracer_get_source(t)).max() > 0.0
                        dev.advance_coupled(2, tracer_only=False, use_limiter=True)
                        assert all(np.isfinite(dev.tracer_get_state(t)).all() for t in range(2)), (name, variant, j)
                        n_launch += 2*(3 + 6 + 1 + 6)*2
            if variant == 'sediment':
                # suspended sediment + Exner (csrc/swe2d_sediment.hip): the coefficient kernel reads the state planes, the cell
                # vertices and the bathymetry and writes the E / D / equilibrium planes; the facet kernel writes the tracer's per-facet
                # value table over the boundary-cell list; the source kernel runs in front of every stage launch (whole mesh, ragged
                # sub-ranges, ForwardEuler); the Exner kernel gathers over the vertex -> (cell, node) list, reads the cell areas and
                # writes the second bathymetry array.  Both forms, a plain tracer next to the field, the batch.  Quadrilaterals: refused.
                # Bedload (swe_bedload_kernel): reads the state planes, the cell vertices, the bathymetry, the gradient table, the areas
                # and the facet codes, writes the six q_b and three contribution planes, which the Exner kernel gathers: every switch
                # combination next to the sediment field, the launch fused with the coefficient pass, the batch, and a handle with
                # bedload alone stepped by swe2d_advance.
                # Slide (swe_slide_kernel): reads the cell vertices, the bathymetry, the gradient table, the areas and the per-cell region,
                # writes the alpha and beta planes and three contribution planes, which the Exner kernel gathers as a third sum: next to
                # sediment + bedload with and without a region, the batch, after the other two are cleared on a handle stepped by
                # swe2d_advance (swe_exner_kernel<false, false, true>), and with bedload alone.
                from thetis_amd.sediment_model import (bedload_constants, bedload_device_parameters, device_parameters,
                                                       sediment_constants, slide_constants, slide_device_parameters)
                cs = sediment_constants(160e-6, 0.025, 1e-6, morfac=50.0)
                plain = dev.add_tracer()
                tid = dev.add_tracer()
                if k == 4:
                    try:
                        dev.sediment_set(tid, device_parameters(cs, False, True))
                        raise AssertionError('the sediment model on quadrilaterals')
                    except _lib.Swe2dError as e:
                        assert e.code == _lib.ERR_UNSUPPORTED
                else:
                    third = mesh.num_cells//3 + 1
                    for conservative in (False, True):
                        dev.sediment_set(tid, device_parameters(cs, conservative, True))
                        dev.sediment_set_equilibrium_bc(markers[0])
                        dev.tracer_set_diffusivity(tid, 0.5)
                        dev.tracer_set_diffusion_bc(tid, markers[0], 4, 0.0)
                        dev.sediment_update()
                        E, D, eq = dev.sediment_read()
                        assert np.isfinite(E).all() and np.isfinite(D).all() and (D > 0).all(), (name, variant)
                        dev.tracer_set_state(tid, eq*(20.0 if conservative else 1.0))
                        dev.tracer_set_state(plain, np.ones((mesh.num_cells, k)))
                        for i in range(3):
                            dev.tracer_solve_stage(tid, i)
                        for i in range(3):
                            dev.tracer_solve_stage_cells(tid, i, 0, third)
                            dev.tracer_solve_stage_cells(tid, i, third, mesh.num_cells)
                        dev.tracer_forward_euler(tid)
                        dev.tracer_limit(tid)
                        dev.exner_step()
                        dev.advance_coupled(2, tracer_only=False, use_limiter=True)
                        assert np.isfinite(dev.tracer_get_state(tid)).all() and np.isfinite(dev.get_bathymetry()).all(), (name, variant)
                        assert np.isfinite(dev.sediment_read_bc()).all() and np.isfinite(dev.tracer_get_source(tid)).all()
                        dev.exner_skipped()
                        for sw in range(8):
                            cb = bedload_constants(cs, 1.3, 2/3, 0.75, bool(sw & 1), bool(sw & 2), bool(sw & 4))
                            for fuse in (0, 1):
                                dev.bedload_set(dict(bedload_device_parameters(cb, True), fuse_with_sediment=fuse), markers[:1])
                                dev.sediment_update()
                                dev.bedload_update()
                                dev.exner_step()
                                n_launch += 4
                                assert all(np.isfinite(a).all() for a in dev.bedload_read()), (name, variant, sw, fuse)
                            dev.advance_coupled(2, tracer_only=False, use_limiter=True)
                            n_launch += 2*(3 + 6 + 2 + 6 + 3 + 1 + 1)
                        assert np.isfinite(dev.get_bathymetry()).all(), (name, variant)
                        sl = slide_device_parameters(slide_constants(cs, 1.0, 0.2, 0.4, 50.0), True)
                        for region in (None, np.where(np.arange(mesh.num_cells) % 3 == 0, 0.0, 1.0)):
                            dev.slide_set(sl, region)           # sediment + bedload + slide: swe_exner_kernel<true, true, true>
                            dev.slide_update()
                            dev.exner_step()
                            dev.advance_coupled(2, tracer_only=False, use_limiter=True)
                            n_launch += 2 + 2*(3 + 6 + 2 + 6 + 3 + 1 + 1 + 1)
                            assert all(np.isfinite(a).all() for a in dev.slide_read()), (name, variant)
                            dev.slide_max_angle(), dev.slide_flagged()
                        dev.bedload_clear()                     # sediment + slide: <true, false, true>
                        dev.slide_update()
                        dev.exner_step()
                        dev.bedload_set(bedload_device_parameters(cb, True), markers[:1])
                        assert np.isfinite(dev.get_bathymetry()).all(), (name, variant)
                        dev.sediment_clear()                    # bedload and slide from here: the Exner tables stay, <false, true, true>
                        dev.bedload_update()
                        dev.slide_update()
                        dev.exner_step()
                        dev.advance(2)
                        dev.slide_clear()                       # bedload alone
                        dev.bedload_update()
                        dev.exner_step()
                        dev.advance(2)
                        assert np.isfinite(dev.get_bathymetry()).all() and not dev.flow_supported(), (name, variant)
                        dev.slide_set(sl, None)
                        dev.bedload_clear()                     # slide alone: the gradient table stays, <false, false, true>
                        dev.slide_update()
                        dev.exner_step()
                        dev.advance(2)
                        assert np.isfinite(dev.get_bathymetry()).all() and not dev.flow_supported(), (name, variant)
                        dev.slide_clear()
                        n_launch += 2 + 3 + 2*6 + 2 + 2*5 + 2 + 2*5
                        n_launch += 2 + 3*2 + 6*2 + 2 + 3 + 1 + 2*(3 + 6 + 2 + 6 + 3 + 1)
            if variant == 'sections':
                # section transports (csrc/swe2d_sections.hip): swe_section_transport_kernel reads the piece tables (cell, weights,
                # normals), the state planes, the cell vertices, the bathymetry and the tracers' planes through the checked loads;
                # the limb sums are atomics on host-checked sizes (capacity + 1 rows).  A polyline of more than one workgroup
                # (triangles), every boundary marker, an unused slot, a last workgroup with padding lanes; rows between steps.
                from thetis_amd import sections as sec
                tids = [dev.add_tracer(), dev.add_tracer()]
                for t in tids:
                    dev.tracer_set_state(t, np.ones((mesh.num_cells, k)))
                lo, hi = cxy.reshape(-1, 2).min(axis=0), cxy.reshape(-1, 2).max(axis=0)
                parts = [None] + [sec.boundary_pieces(mesh, m) for m in markers]
                if k == 3:
                    parts.append(sec.cut_polyline(mesh, [lo + 0.01*(hi - lo), hi - 0.02*(hi - lo), lo + (0.9, 0.05)*(hi - lo)]))
                live = [(s_, p_) for s_, p_ in enumerate(parts) if p_ is not None]
                dev.sections_set(len(parts), np.concatenate([np.full(len(p_), s_) for s_, p_ in live]),
                                 np.concatenate([p_.cell for _, p_ in live]), np.concatenate([p_.weights for _, p_ in live]),
                                 np.concatenate([p_.normal for _, p_ in live]), tids)
                dev.sections_rows_reserve(3)
                for _ in range(3):
                    dev.advance_coupled(1, tracer_only=False, use_limiter=True)
                    dev.sections_rows_append()
                rows, bad = dev.sections_rows_read()
                values, bad_now = dev.sections_eval()
                assert len(rows) == 3 and not bad.any() and bad_now == 0 and np.isfinite(rows).all(), (name, variant)
                assert np.array_equal(rows[2], values) and (values[1:len(parts), 1] > 0).all() and not values[0].any()
                n_launch += 3*(3 + 6 + 1) + 4
            dev.advance(2)
            dev.advance_forward_euler(1)
            for i in range(3):                      # sub-range launches with ragged ends
                dev.solve_stage_cells(i, 0, mesh.num_cells//3 + 1)
                dev.solve_stage_cells(i, mesh.num_cells//3 + 1, mesh.num_cells)
            if dev.flow_supported():                # the dataflow launch (plane accesses are checked; granules use a bounded resource)
                dev.solve_flow([mesh.num_cells]*6)
                n_launch += 1
            if variant in ('plain', 'open+fields', 'sources'):
                # round 6: the fused stage kernels (csrc/swe2d_fuse.h: the tile tables are host-built indices into LDS and memory) -
                # stages 1 + 2 in one launch on triangles and quadrilaterals, all three on triangles, forced on these small meshes
                dev.set_option(_lib.OPT_FLOW, 0)
                for mode in ((1, 3, 33) if k == 3 else (1,)):
                    if mode == 33:                   # the two-ring tiles as patches (structured meshes: 5 x 3 quads; else bisection leaves of 40 cells)
                        mode = 3
                        tiles = ordering.triple_tile_order(mesh, 5, 3)
                        if tiles is None:
                            cen = mesh.cell_xy().mean(axis=1)
                            tiles = (ordering.bisection_block_order(cen, block=40), np.arange(0, mesh.num_cells, 40))
                        dev.fused_set_triple_tiles(*tiles)
                    dev.set_option(_lib.OPT_FUSED_STAGES, mode)
                    assert dev.fused_pair_info()[0] and (mode != 3 or dev.fused_triple_info()[0]), (name, variant, mode)
                    dev.advance(3)
                    n_launch += 6
                dev.set_option(_lib.OPT_FUSED_STAGES, None)
                dev.set_option(_lib.OPT_FLOW, None)
            dev.tendency()
            d = dev.diagnostics()
            assert np.isfinite(d).all(), (name, variant, d)
            dev.get_state()
            dev.close()
            n_launch += 30
            print('ok', name, variant, flush=True)
    if only:
        return n_launch
    # partitions: halo cells, owned / interior sub-ranges, pack / unpack
    from thetis_amd.partition import build_partition, rcb_owner
    mesh, bath, uv, eta = channel_case(nx=23, ny=11, seed=4)
    owner = rcb_owner(mesh, 3)
    for rank in range(3):
        p = build_partition(mesh, owner, rank)
        dev = Swe2dDevice(p, np.asarray(bath)[p.vertex_global], 0.05, n_owned=p.n_owned, boundary_len=p.boundary_len,
                          ranges=p.reorder_ranges())
        dev.halo_setup(p.send_cells, p.recv_cells)
        dev.set_state(0.1*uv[p.local_to_global], 0.1*eta[p.local_to_global])
        for i in range(3):
            inner = p.owned_prefix(3)
            dev.solve_stage_cells(i, 0, inner)
            dev.solve_stage_cells(i, inner, p.stage_range(i))
        # the fused stage pair on the partition's ranges (tiles cut from an order that mixes owned and ghost cells)
        from thetis_amd import ordering
        dev.set_option(_lib.OPT_FUSED_STAGES, 1)
        dev.fused_set_order(ordering.fused_tile_order(p))
        assert dev.fused_pair_info()[0]
        dev.solve_stage_pair_cells(p.stage_range(0), p.stage_range(1))
        dev.solve_stage_cells(2, 0, p.n_owned)
        # ... and whole steps in one launch each on the partition's two-ring tiles, cut as patches of the parent mesh (5 x 3 quads here),
        # the state buffers changing places (swe2d_solve_step_cells)
        dev.set_option(_lib.OPT_FUSED_STAGES, 3)
        tiles = ordering.triple_tile_order(p, 5, 3)
        if tiles is not None:
            dev.fused_set_triple_tiles(*tiles)
        assert dev.fused_step_info()[0]
        dev.solve_step_cells(p.n_owned)
        dev.diagnostics()
        dev.close()
        n_launch += 10
    print('ok partitions', flush=True)
    return n_launch


def main():
    from thetis_amd import _lib
    selftest = os.environ.get('THETIS_AMD_RANGE_SELFTEST') == '1'
    # python tools/range_check.py [variant,variant,...]: only these variants (and no partitions)
    only = set(sys.argv[1].split(',')) if len(sys.argv) > 1 else None
    n_launch = 0
    try:
        n_launch = exercise(only)
    except Exception as e:                       # the negative control suppresses accesses: non-finite states are expected there
        if not selftest:
            raise
        print('negative control stopped at:', e)
    out = (ctypes.c_ulonglong*5)()
    lib = _lib.load()
    if not hasattr(lib, 'swe2d_debug_range_report'):
        raise SystemExit('not a -DSWE_RANGE_CHECK build: ' + _lib.LIB_PATH)
    lib.swe2d_debug_range_report.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    assert lib.swe2d_debug_range_report(out) == 0
    print('range check: ~{:d} launches, {:d} checked launches, {:d} violations{}'.format(
        n_launch, out[3], out[0], '' if not out[0] else ' (first: address 0x{:x}, swe2d_kernels.h/swe2d_sipg.h line {:d})'.format(out[1], out[2])))
    if selftest:
        sys.exit(0 if out[0] > 0 else 'negative control found no violation')
    sys.exit(1 if out[0] else 0)


if __name__ == '__main__':
    main()
