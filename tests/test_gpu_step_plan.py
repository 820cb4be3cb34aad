"""
How a step is launched (csrc/swe2d_plan.hip), as a decision table: for every setting of SWE2D_OPT_FUSED_STAGES, SWE2D_OPT_FLOW and
SWE2D_OPT_BND_INLINE and five configurations, on 1600 triangles (with and without the caller's two-ring patches) and 1600
parallelograms - what swe2d_flow_supported and the three swe2d_fused_*_info calls answer, which stage buffers swe2d_advance leaves
readable, and that swe2d_advance gives the bits of swe2d_solve_stage x 3.

The expectations are the rules of include/swe2d.h (swe2d_option, swe2d_fused_*_info, swe2d_flow_supported, swe2d_get_stage_state)
written out for a whole mesh of 1600 cells: far below every size from which a tile kernel is taken by itself (250 k / 850 k / 131 073 /
2.5 M cells, covered at size by tests/test_gpu_parity.py), above the 64 cells from which a forced mode applies, and within what the
dataflow kernel holds.
"""
import itertools

import numpy as np
import pytest

from helpers import channel_case, quad_case

pytestmark = pytest.mark.gpu

KINDS = ['triangles', 'triangles_patches', 'parallelograms']
# configuration -> (swe2d_flow_supported on triangles: 0 not covered | 1 covered | 2 covered and without source terms,
#                   the tile kernels - stage pair, three-stage kernel - cover it)
CONFIGS = {
    'plain':          (2, True),
    'manning':        (1, True),      # source terms: covered by every kernel (the three-stage kernel only declines them by itself)
    'viscosity':      (0, False),
    'wetting_drying': (2, False),     # the dataflow kernel carries it (nonlinear equations, SWE2D_OPT_FLOW_WD unset), the tiles do not
    'farm':           (0, False),     # tidal turbine farms: the stage kernels alone
}
# SWE2D_OPT_FUSED_STAGES at 1600 cells -> (the stage pair is taken, the three-stage kernel is taken) where the kernels cover the handle:
# by itself (unset) and 2 only from 250 k cells, 1 forces the pair, 3 the three-stage kernel (and the pair where that one does not apply:
# quadrilaterals, a whole-mesh step inside a stream capture)
FUSED = {None: (False, False), 0: (False, False), 1: (True, False), 2: (False, False), 3: (True, True)}
FLOW = [None, 0]
BND_INLINE = [None, 0]                # 0: the epilogue variant of the stage kernels, which keeps the tile and the dataflow kernels away


def expected(kind, config, fused, flow, bnd_inline):
    """(flow_supported, fused_pair_info[0], fused_triple_info[0], fused_step_info[0]), readable stage buffers (U(1), U(2)) after advance"""
    tri = kind != 'parallelograms'
    flow_cfg, tiles_cfg = CONFIGS[config]
    flow_supported = flow_cfg if (tri and bnd_inline != 0) else 0
    pair, triple = FUSED[fused]
    pair = pair and tiles_cfg and bnd_inline != 0
    triple = triple and tiles_cfg and bnd_inline != 0 and tri
    advance_by_flow = flow_supported != 0 and flow != 0       # only swe2d_advance takes it, before every tile kernel
    # swe2d_fused_pair_info: 0 where the dataflow kernel takes the whole mesh; swe2d_fused_triple_info / _step_info do not look at it
    infos = (flow_supported, int(pair and not advance_by_flow), int(triple), int(triple))
    if advance_by_flow or triple:
        readable = (False, False)                             # U(1) and U(2) never leave the chip
    elif pair:
        readable = (False, True)                              # U(1) stays on chip, buffer C holds U(2)
    else:
        readable = (True, True)                               # three stage launches
    return infos, readable


def _case(kind):
    if kind == 'parallelograms':
        mesh, bath, uv, eta = quad_case(nx=40, ny=40, seed=11, skew=0.3)
    else:
        mesh, bath, uv, eta = channel_case(nx=40, ny=20, seed=11)
    assert mesh.num_cells == 1600
    return mesh, bath, 0.2*uv, 0.2*eta


def _configure(dev, mesh, config):
    from thetis_amd import _lib
    if config == 'manning':
        dev.set_scalar(_lib.SCALAR_MANNING_DRAG, 0.02)
    elif config == 'viscosity':
        dev.set_viscosity(30.0)
    elif config == 'wetting_drying':
        dev.set_wetting_and_drying(0.5)
    elif config == 'farm':
        xc = mesh.cell_xy()[:, :, 0].mean(axis=1)
        density = np.where(((xc > 30e3) & (xc < 70e3))[:, None], 1e-5, 0.0)*np.ones((1, mesh.cells.shape[1]))
        p = _lib.TurbineParams()
        p.rotor_area = p.projected_diameter = 18.0
        p.thrust_area_const = 0.8*18.0
        p.power_const = 0.4
        p.rho0 = 1000.0
        dev.turbine_farm_set(0, p, density)


@pytest.mark.parametrize('config', list(CONFIGS))
@pytest.mark.parametrize('kind', KINDS)
def test_decision_table(hip_lib, kind, config):
    from thetis_amd import _lib, ordering
    from thetis_amd.device import Swe2dDevice
    mesh, bath, uv, eta = _case(kind)
    dev = Swe2dDevice(mesh, bath, 2.0)
    if kind == 'triangles_patches':
        dev.fused_set_triple_tiles(*ordering.triple_tile_order(mesh, 11, 8))
    _configure(dev, mesh, config)
    for opt in (_lib.OPT_FUSED_STAGES, _lib.OPT_FLOW, _lib.OPT_BND_INLINE, _lib.OPT_FLOW_WD):
        dev.set_option(opt, None)                             # the handle's own rule unless a row says otherwise (not the environment)
    dev.set_state(uv, eta)
    dev.snapshot()
    for _ in range(2):
        for i in range(3):
            dev.solve_stage(i)
    ref = dev.get_state()
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for fused, flow, bnd_inline in itertools.product(FUSED, FLOW, BND_INLINE):
        row = (kind, config, fused, flow, bnd_inline)
        dev.set_option(_lib.OPT_FUSED_STAGES, fused)
        dev.set_option(_lib.OPT_FLOW, flow)
        dev.set_option(_lib.OPT_BND_INLINE, bnd_inline)
        infos, readable = expected(*row)
        got = (dev.flow_supported(), dev.fused_pair_info()[0], dev.fused_triple_info()[0], dev.fused_step_info()[0])
        assert got == infos, (row, got, infos)
        dev.restore()
        dev.advance(2)
        for i in (0, 1):
            if readable[i]:
                dev.get_state(i)
            else:
                with pytest.raises(_lib.Swe2dError) as err:
                    dev.get_state(i)
                assert err.value.code == _lib.ERR_UNSUPPORTED, row
        out = dev.get_state()
        assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]), row
    dev.close()
