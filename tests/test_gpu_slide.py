"""The sediment slide on the device (swe_slide_kernel and swe_exner_kernel<.., .., true>, csrc/swe2d_sediment.hip) against
thetis_amd/sediment_model.py's HostSediment: alpha and beta to the rounding of the two math libraries with the same set of sliding
cells; the contribution planes and the Exner update bit for bit from the device's own alpha plane, alone, with bedload and with
sediment + bedload; the maximum angle and the flagged count; batches against the step-by-step loop; clear; the region."""
import numpy as np
import pytest

from bedload_cases import ALPHA_SECC, BETA, SURBETA2, bedload_state
from sediment_cases import mesh_case
from slide_cases import DT, MORFAC, slide_c, steep_bed
from thetis_amd.device import Swe2dDevice
from thetis_amd.sediment_model import (HostSediment, bedload_constants, bedload_device_parameters, device_parameters,
                                       slide_device_parameters)

pytestmark = pytest.mark.gpu

# (mesh, seed, quantile of tests/slide_cases.steep_bed): beds whose steepest cell stays below 41 degrees, away from the zero of the
# reference's cos(beta*dt*morfac) = cos(2 beta) at 45 degrees, where 1/cos turns one ulp of asin into many of alpha
BEDS = {'channel': (4, 0.5), 'coast': (7, 0.5), 'large': (4, 0.7), 'v63': (5, 0.5), 'v64': (4, 0.7), 'v65': (4, 0.7), 'jack': (0, 0.7)}

# Largest difference between the device and numpy (asin and cos are the device library's), measured on the MI355X over the seven beds
# above (profiles/r19c_slide_gpu_measurements.txt): alpha relative to max |alpha| 1.12e-15 (coast), 1.07e-15 (v65),
# 9.8e-16 (5000 triangles), at most 1.1e-16 elsewhere; beta relative to max beta 1.75e-16 (v65) at most.
# Asserted: ten times the largest, and never more than the cap of 1e-12 that tells a wrong formula from rounding.
MEASURED_ALPHA = 1.2e-15
MEASURED_BETA = 1.8e-16
ALPHA_BOUND = min(10*MEASURED_ALPHA, 1e-12)
BETA_BOUND = min(10*MEASURED_BETA, 1e-12)


def _constants(morfac=MORFAC):
    return bedload_constants(slide_c(morfac=morfac), BETA, SURBETA2, ALPHA_SECC, True, True, False)


def _bed(name):
    mesh = mesh_case(name)
    seed, q = BEDS[name]
    return mesh, steep_bed(mesh, seed, quantile=q)


def _setup(name, c, reorder='auto', bath=None, with_sediment=False, bedload=False, region=None, solve_exner=False, slide=True):
    mesh, b = _bed(name)
    bath = b if bath is None else bath
    bath0, uv, eta = bedload_state(mesh, seed=1, smooth=True)
    eta = eta + bath0[mesh.cells] - bath[mesh.cells]                             # the nodal depths of the state on this bed
    dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len, reorder=reorder)
    tid = None
    if with_sediment:
        tid = dev.add_tracer()
        dev.sediment_set(tid, device_parameters(c, False, solve_exner))
    if bedload:
        dev.bedload_set(bedload_device_parameters(c, solve_exner), list(mesh.boundary_markers)[:1])
    if slide:
        dev.slide_set(slide_device_parameters(c, solve_exner), region)
    dev.set_state(uv, eta)
    return mesh, bath, uv, eta, dev, tid


def _host_like_device(dev, c):
    """HostSediment in the device's numbering and the maps caller -> device of cell and vertex arrays, device -> caller of vertex
    arrays"""
    host = HostSediment(dev._keep[0], dev._keep[1], c)
    nodal = (lambda a: a[dev.perm]) if dev.perm is not None else (lambda a: a)
    vert = (lambda b: b[dev._vperm]) if dev._vperm is not None else (lambda b: b)

    def back(b):
        if dev._vperm is None:
            return b
        out = np.empty_like(b)
        out[dev._vperm] = b
        return out
    return host, dev._keep[2], nodal, vert, back


def _check_planes(name, reorder):
    c = _constants()
    mesh, bath, uv, eta, dev, _ = _setup(name, c, reorder=reorder)
    dev.slide_update()
    alpha, beta, contrib = dev.slide_read()
    hd, _, nodal, vert, _ = _host_like_device(dev, c)
    wa, wb, wc, wf = hd.slide(vert(bath), DT)
    ga, gb = nodal(alpha), nodal(beta)
    assert np.isfinite(ga).all() and np.isfinite(gb).all() and (wa != 0).any() and (wa == 0).any()
    assert np.array_equal(ga != 0, wa != 0)                                      # the same cells slide: sqrt and division only
    assert np.array_equal(gb == 0, wb == 0)
    ea, eb = np.abs(ga - wa).max()/np.abs(wa).max(), np.abs(gb - wb).max()/wb.max()
    print('slide planes {:} {:}: alpha {:.3e} of max |alpha|, beta {:.3e} of max beta, {:d} of {:d} cells slide, {:d} flagged'.format(
        name, reorder, ea, eb, int((wa != 0).sum()), len(wa), wf))
    # from the device's own alpha: contributions, maximum, flags - exact
    assert np.array_equal(nodal(contrib), hd.slide_contributions(ga, vert(bath)))
    assert dev.slide_max_angle() == gb.max()
    assert dev.slide_flagged() == int(hd.slide_flags(ga, DT).sum())
    dev.close()
    return ea, eb


@pytest.mark.parametrize('name,reorder', [('channel', None), ('channel', 'auto'), ('coast', 'auto'), ('coast', None), ('large', 'auto'),
                                          ('v63', None), ('v64', 'auto'), ('v65', 'auto'), ('jack', None)])
def test_alpha_and_beta_against_the_replay(name, reorder):
    ea, eb = _check_planes(name, reorder)
    assert ea <= ALPHA_BOUND and eb <= BETA_BOUND


def test_a_flat_bed_and_a_cell_exactly_at_the_angle():
    """a bed flat to the last bit: alpha = 0 and beta = 0 exactly, nothing is NaN, the bed stays.  The angle of repose set to the very
    tangent one cell computes: tanbeta - tanphi = 0 there, and the cell does not slide (the select is strict)"""
    c = _constants()
    mesh = mesh_case('coast')
    for level in (0.0, 0.7):
        mesh, bath, uv, eta, dev, _ = _setup('coast', c, bath=np.full(mesh.vertex_xy.shape[0], level))
        dev.slide_update()
        alpha, beta, contrib = dev.slide_read()
        assert not alpha.any() and not beta.any() and not contrib.any() and not np.isnan(alpha).any()
        assert dev.slide_max_angle() == 0.0 and dev.slide_flagged() == 0
        if level:
            dev.exner_step()
            assert np.array_equal(dev.get_bathymetry(), bath)
        dev.close()
    mesh, bath = _bed('channel')
    host = HostSediment(mesh.cells, mesh.vertex_xy, c)
    bx, by = host.gradient(bath[mesh.cells])
    nz = 1.0/np.sqrt(1.0 + (bx*bx + by*by))
    tanbeta = np.sqrt(1.0 - nz*nz)/nz
    k = int(np.argsort(tanbeta)[len(tanbeta)//2])
    at = dict(c, tanphi=float(tanbeta[k]))
    mesh, bath, uv, eta, dev, _ = _setup('channel', at, reorder=None)
    dev.slide_update()
    alpha = dev.slide_read()[0]
    assert alpha[k] == 0.0 and np.array_equal(alpha != 0, tanbeta > tanbeta[k]) and (alpha != 0).any()
    dev.close()


@pytest.mark.parametrize('name,with_sediment,bedload,reorder', [
    ('v63', False, False, None), ('v64', False, True, 'auto'), ('v65', True, True, 'auto'), ('jack', False, False, None),
    ('jack', True, True, None), ('large', False, False, 'auto'), ('large', True, True, None), ('channel', False, True, 'auto'),
    ('coast', False, False, None), ('coast', True, True, 'auto')])
def test_contributions_and_exner_bit_for_bit(name, with_sediment, bedload, reorder):
    """from the device's own alpha plane (and its own q_b and coefficient planes): the contribution planes and the bed update of
    HostSediment in the device's cell and vertex order, bit for bit; slide alone, with bedload, with sediment + bedload"""
    c = _constants()
    mesh, bath, uv, eta, dev, tid = _setup(name, c, reorder=reorder, with_sediment=with_sediment, bedload=bedload)
    hd, nbr, nodal, vert, back = _host_like_device(dev, c)
    dev.slide_update()
    alpha, beta, contrib = dev.slide_read()
    want_s = hd.slide_contributions(nodal(alpha), vert(bath))
    assert np.array_equal(nodal(contrib), want_s) and np.abs(want_s).max() > 0
    want_b = None
    if bedload:
        dev.bedload_update()
        qx, qy, cb = dev.bedload_read()
        mask = 1 << dev._slot(list(mesh.boundary_markers)[0])
        want_b = hd.bedload_contributions(np.stack([nodal(qx), nodal(qy)], axis=2), nbr, mask)
        assert np.array_equal(nodal(cb), want_b)
    E = D = S = None
    if with_sediment:
        dev.sediment_update()
        E, D, eq = dev.sediment_read()
        S = 0.5*eq
        dev.tracer_set_state(tid, S)
        E, D, S = nodal(E), nodal(D), nodal(S)
    want = back(hd.exner(E, D, S, nodal(eta), vert(bath), DT, bedload=want_b, slide=want_s))
    dev.exner_step()
    got = dev.get_bathymetry()
    assert np.array_equal(got, want) and (got != bath).sum() > len(bath)//10
    assert dev.exner_skipped() == hd.n_skipped
    assert (want != back(hd.exner(E, D, S, nodal(eta), vert(bath), DT, bedload=want_b))).any()       # (the slide did change the update)
    dev.close()


def test_a_region_of_zeros_on_half_the_mesh():
    c = _constants()
    mesh, bath = _bed('large')
    region = np.where(mesh.vertex_xy[mesh.cells][..., 0].mean(axis=1) < 8.0, 0.0, 1.0)
    mesh, bath, uv, eta, dev, _ = _setup('large', c, region=region)
    dev.slide_update()
    alpha, beta, contrib = dev.slide_read()
    off = region == 0.0
    assert 0.3 < off.mean() < 0.7 and not alpha[off].any() and not beta[off].any() and not contrib[off].any() and alpha[~off].any()
    dev.slide_set(slide_device_parameters(c, False), None)                        # the region goes, the parameters stay
    dev.slide_update()
    full = dev.slide_read()
    assert full[0][off].any() and np.array_equal(full[0][~off], alpha[~off]) and np.array_equal(full[2][~off], contrib[~off])
    hd, _, nodal, vert, _ = _host_like_device(dev, c)
    assert np.array_equal(nodal(alpha) != 0, hd.slide(vert(bath), DT, nodal(region))[0] != 0)
    dev.close()


def _ramp_device(c, with_sediment, bedload, slide, solve_exner=True):
    """the channel with a steep bump in the flow of the bedload tests"""
    mesh = mesh_case('channel')
    x = mesh.vertex_xy[:, 0]
    bath = 0.9 + 0.6*np.exp(-((x - 8.0)/1.5)**2)                                 # slopes of 0.1 - 0.25 across the cells of the bump
    n = mesh.num_cells
    uv = np.zeros((n, 3, 2))
    uv[..., 0] = 0.5*0.9/bath[mesh.cells]
    eta = 0.002*np.cos(mesh.vertex_xy[mesh.cells][..., 0]/3.0)
    dev = Swe2dDevice(mesh, bath, 0.02, boundary_len=mesh.boundary_len)
    tid = None
    if with_sediment:
        tid = dev.add_tracer()
        dev.sediment_set(tid, device_parameters(c, False, solve_exner))
        dev.tracer_set_options(False, 1.0, 1.0)
        dev.sediment_set_equilibrium_bc(1)
        dev.tracer_set_state(tid, np.zeros((n, 3)))
    if bedload:
        dev.bedload_set(bedload_device_parameters(c, solve_exner), [1, 2])
    if slide:
        dev.slide_set(slide_device_parameters(dict(c, tanphi=0.1), solve_exner), None)
    dev.set_bc(1, {'uv': (0.5, 0.0)})
    dev.set_bc(2, {'elev': 0.0})
    dev.set_state(uv, eta)
    return mesh, bath, dev, tid


def _result(dev, tid):
    return dev.get_state() + ((dev.tracer_get_state(tid),) if tid is not None else ()) + (dev.get_bathymetry(),)


@pytest.mark.parametrize('with_sediment,bedload,limiter', [(True, True, True), (True, False, False), (False, True, False),
                                                            (False, False, False)])
def test_batches_equal_the_step_by_step_loop(with_sediment, bedload, limiter):
    """8 steps in one call against the loop of single launches in the order flow, sediment stages, limiter, bedload, slide, Exner:
    state, sediment and bed bit for bit, and the maximum angle and the flagged count with them.  A handle without a sediment field
    takes swe2d_advance as well as swe2d_advance_coupled."""
    c = _constants(morfac=50.0)
    out = []
    for mode in ('coupled', 'loop') + (() if with_sediment else ('advance',)):
        mesh, bath, dev, tid = _ramp_device(c, with_sediment, bedload, True)
        assert not dev.flow_supported()                                          # never the multi-step dataflow kernel
        if mode == 'coupled':
            dev.advance_coupled(8, tracer_only=False, use_limiter=limiter)
        elif mode == 'advance':
            dev.advance(8)
        else:
            for _ in range(8):
                for i in range(3):
                    dev.solve_stage(i)
                if with_sediment:
                    dev.sediment_update()
                    for i in range(3):
                        dev.tracer_solve_stage(tid, i)
                    if limiter:
                        dev.tracer_limit(tid)
                if bedload:
                    dev.bedload_update()
                dev.slide_update()
                dev.exner_step()
        res = _result(dev, tid) + dev.slide_read() + (np.array([dev.slide_max_angle(), dev.slide_flagged()]),)
        assert all(np.isfinite(a).all() for a in res) and np.abs(res[len(res) - 5] - bath).max() > 0 and np.abs(res[-4]).max() > 0
        out.append(res)
        dev.close()
    for other in out[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(out[0], other))


@pytest.mark.parametrize('with_sediment', [True, False])
def test_after_slide_clear_the_handle_is_one_that_never_had_it(with_sediment):
    """sediment + bedload (or bedload alone) with the slide set, evaluated and cleared against a handle that never had it: the same
    bits after 4 steps - those of swe_exner_kernel<.., true, false>, the instantiations of a handle without slide; with the slide
    the bed moves differently"""
    c = _constants(morfac=50.0)
    res = []
    for had_slide in (True, False):
        mesh, bath, dev, tid = _ramp_device(c, with_sediment, True, had_slide)
        if had_slide:
            dev.slide_update()
            assert np.abs(dev.slide_read()[0]).max() > 0
            dev.slide_clear()
            with pytest.raises(Exception, match='swe2d_slide_set'):
                dev.slide_update()
        dev.advance_coupled(4, tracer_only=False, use_limiter=True)
        res.append(_result(dev, tid))
        dev.close()
    assert all(np.array_equal(p, q) for p, q in zip(*res)) and np.abs(res[0][-1] - bath).max() > 0
    mesh, bath, dev, tid = _ramp_device(c, with_sediment, True, True)
    dev.advance_coupled(4, tracer_only=False, use_limiter=True)
    assert (dev.get_bathymetry() != res[0][-1]).any()
    dev.close()


def test_plan_and_table_ownership():
    """a handle with slide never gets the dataflow plan; the gradient table and the Exner tables outlive whichever model is cleared
    first"""
    c = _constants()
    mesh, bath = _bed('large')
    dev = Swe2dDevice(mesh, bath, DT, boundary_len=mesh.boundary_len)
    assert dev.flow_supported()
    dev.slide_set(slide_device_parameters(c, False))
    assert not dev.flow_supported()
    dev.slide_clear()
    assert dev.flow_supported()
    dev.bedload_set(bedload_device_parameters(c, True))
    dev.slide_set(slide_device_parameters(c, True))
    dev.bedload_clear()                                                          # slide alone from here on: the tables stay
    dev.slide_update()
    alpha, beta, contrib = dev.slide_read()
    dev.exner_step()
    hd, _, nodal, vert, back = _host_like_device(dev, c)
    eta = np.zeros((mesh.num_cells, 3))
    want = back(hd.exner(None, None, None, eta, vert(bath), DT, slide=nodal(contrib)))
    assert np.array_equal(dev.get_bathymetry(), want) and np.abs(want - bath).max() > 0
    dev.bedload_set(bedload_device_parameters(c, True))
    dev.slide_clear()                                                            # and the other way round
    dev.bedload_update()
    assert np.isfinite(dev.bedload_read()[2]).all()
    dev.close()
