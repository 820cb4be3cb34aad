"""CPU: what the seeds of tests/test_gpu_fuzz_paths.py draw (tests/fuzz_cases.py) - a randomised test must not pass because a
kind of boundary, a source term or a tiling never came up - and that moving the generator out of tests/test_gpu_fuzz.py left
the draws of its seeds alone."""
import collections

import numpy as np
import pytest

import fuzz_cases as fc
from thetis_amd import _lib

# fc.options_digest over seeds 0-191 of tests/test_gpu_fuzz.py::_random_config as it stood before the move (computed from that
# file's text, not from fuzz_cases.random_config)
PARENT_DIGEST = 'd7543c8390bc6da20ff99ac86c2a463259e926746e3228de654db05980f05f61'


def test_moved_generator_draws_what_it_drew():
    assert fc.options_digest(fc.legacy_case(s)[4] for s in range(192)) == PARENT_DIGEST
    assert any(fc.legacy_case(s)[7] for s in range(192))                                  # wetting-drying is still drawn there
    assert any('horizontal_viscosity' in fc.legacy_case(s)[4] for s in range(192))


def test_digest_sees_every_value():
    o = fc.legacy_case(5)[4]
    base = fc.options_digest([o])
    for key in o:
        if isinstance(o[key], dict):
            continue
        changed = dict(o)
        changed[key] = (not o[key]) if isinstance(o[key], bool) else np.asarray(o[key], dtype=float)*(1 + 1e-15) + 1e-300
        assert fc.options_digest([changed]) != base, key
    assert fc.options_digest([dict(o, extra=1.0)]) != base


@pytest.fixture(scope='module')
def cases():
    return ([fc.path_case(s) for s in fc.TRI_SEEDS] + [fc.quad_path_case(s) for s in fc.QUAD_SEEDS]
            + [fc.partition_case(s) for s in fc.PARTITION_SEEDS])


def test_restricted_draw_has_nothing_the_tile_kernels_decline(cases):
    for c in cases:
        assert 'use_wetting_and_drying' not in c['o'] and 'horizontal_viscosity' not in c['o']
        assert {op[0] for op in c['dev_ops']} <= {'set_field', 'set_scalar'}


def test_every_kind_of_boundary_source_and_drag_is_drawn(cases):
    n = collections.Counter()
    for c in cases[:len(fc.TRI_SEEDS) + len(fc.QUAD_SEEDS)]:
        o, ops, bcs = c['o'], c['dev_ops'], c['bcs']
        for marker in (1, 2, 3, 4):
            funcs = bcs.get(marker, {})
            n['kind', tuple(sorted(k for k in funcs if k != 'drag'))] += 1
            for key, val in funcs.items():
                if key == 'drag':
                    n['bnd_drag'] += 1
                else:
                    n[key, 'field' if np.ndim(val) >= 2 else 'const'] += 1
        if any('drag' in f for f in bcs.values()) and not fc.has_sources(ops):
            n['bnd_drag_without_sources'] += 1
        for key in fc.SOURCE_FIELDS:
            n[key] += key in o
        fields = {op[1][0] for op in ops if op[0] == 'set_field'}
        scalars = {op[1][0] for op in ops if op[0] == 'set_scalar'}
        n['drag', 1] += _lib.SCALAR_QUADRATIC_DRAG in scalars
        n['drag', 2] += _lib.SCALAR_MANNING_DRAG in scalars
        n['drag', 3] += _lib.SCALAR_NIKURADSE in scalars
        n['drag', 4] += _lib.FIELD_MANNING_DRAG in fields
        n['drag', 5] += _lib.FIELD_QUADRATIC_DRAG in fields
        n['linear const'] += _lib.SCALAR_LINEAR_DRAG in scalars
        n['linear field'] += _lib.FIELD_LINEAR_DRAG in fields
        n['smoother'] += _lib.SCALAR_NORM_SMOOTHER in scalars
        n['lf 0.6'] += o['lax_friedrichs_velocity_scaling_factor'] == 0.6
        n['nonlin', o['use_nonlinear_equations']] += 1
        n['lf', o['use_lax_friedrichs_velocity']] += 1
        n['mesh', c['kind']] += 1
        n['reorder', c['reorder']] += 1
        n['patch', c['patch']] += 1
    for kind in fc.KINDS:
        assert n['kind', tuple(sorted(kind or {}))] >= 1, kind
    for key in ('elev', 'uv', 'un', 'flux'):
        assert n[key, 'const'] >= 5 and n[key, 'field'] >= 5, (key, n)
    assert n['bnd_drag'] >= 5 and n['bnd_drag_without_sources'] >= 2, n
    for key in fc.SOURCE_FIELDS:
        assert n[key] >= 5, key
    for kind in range(1, 6):
        assert n['drag', kind] >= 5, kind
    for key in ('linear const', 'linear field', 'smoother', 'lf 0.6'):
        assert n[key] >= 5, key
    for flag in (True, False):
        assert n['nonlin', flag] >= 1 and n['lf', flag] >= 1
    for kind in fc.TRI_MESH_KINDS + fc.QUAD_MESH_KINDS:
        assert n['mesh', kind] >= 1, kind
    for reorder in fc.REORDERS:
        assert n['reorder', reorder] >= 1, reorder
    for patch in fc.PATCHES:
        assert n['patch', patch] >= 1, patch


def test_perturbation_keeps_the_kinds_and_changes_the_values(cases):
    changed_field = changed_scalar = 0
    for c in cases:
        assert set(c['bcs2']) == set(c['bcs'])
        for marker, funcs in c['bcs'].items():
            new = c['bcs2'][marker]
            assert list(new) == list(funcs)
            for key in funcs:
                assert np.shape(new[key]) == np.shape(funcs[key])
                assert not np.array_equal(np.asarray(new[key]), np.asarray(funcs[key])), (marker, key)
        old = {(op[0], op[1][0]): op[1][1] for op in c['dev_ops']}
        assert len(c['ops2']) == (any(k[0] == 'set_field' for k in old)
                                  + any(k[0] == 'set_scalar' and k[1] in fc.DRAG_SCALARS for k in old))
        for op in c['ops2']:
            assert np.shape(op[1][1]) == np.shape(old[op[0], op[1][0]]) and not np.array_equal(op[1][1], old[op[0], op[1][0]])
            changed_field += op[0] == 'set_field'
            changed_scalar += op[0] == 'set_scalar'
        assert fc.has_sources(c['dev_ops']) == bool(c['ops2'])
    assert changed_field >= 5 and changed_scalar >= 5


def test_partition_cases_cut_the_last_two_tiles(cases):
    part = cases[-len(fc.PARTITION_SEEDS):]
    assert {c['tile_from_end'] for c in part} == {1, 2}
    assert {c['kind'] for c in part} == set(fc.TRI_MESH_KINDS)
    assert all(0.0 < c['frac'] < 1.0 for c in part)
