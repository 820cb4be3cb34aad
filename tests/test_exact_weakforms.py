"""CPU: the numpy oracle and the C restatement against exactly integrated weak forms (tests/golden/exact_weakforms*.json.gz, written by
tests/golden/make_exact_weakform_golden.py from the reference's UFL text in rational arithmetic: no rounding, no quadrature rule, no
code shared with the oracle).  Pins signs, '+'/'-' sides, boundary externals, the mass inverse, the Shu-Osher update and the exactness
of the oracle's quadrature rules on the polynomial part of the path (linear equations, flat bathymetry, no Lax-Friedrichs velocity).

Bound: the project's own for two float64 evaluations of one operator, rel_linf < 1e-13 (test_numpy_and_c_restatements_agree).
``python tests/test_exact_weakforms.py FILE`` writes the table of measured errors to FILE."""
import collections
import importlib.util
import os
import sys

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exact_cases as ec
from helpers import make_oracle_generic

TOL = 1e-13
NAMES = sorted(ec.cases())


def _generator():
    spec = importlib.util.spec_from_file_location('make_exact_weakform_golden',
                                                  os.path.join(ec.GOLDEN, 'make_exact_weakform_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_file_is_what_the_generator_writes():
    """tri8 case 1 (closed walls) and case 3 (four open boundaries of four kinds) regenerated: same bits of hi and lo, same inputs"""
    gen = _generator()
    doc = gen.build_file('exact_weakforms.json', only=('walls', 'bnd_all_four'))
    committed = ec.documents()['exact_weakforms.json']
    assert sorted(doc['cases']) == ['tri8/bnd_all_four', 'tri8/walls']
    for name, case in doc['cases'].items():
        assert case == committed['cases'][name], name
    assert doc['meshes'] == committed['meshes']


def _data_only(x):
    """numbers, booleans, strings that are float.hex() values or names, lists and dictionaries of them"""
    if isinstance(x, dict):
        return all(isinstance(k, str) and _data_only(v) for k, v in x.items())
    if isinstance(x, list):
        return all(_data_only(v) for v in x)
    if isinstance(x, str):
        if x.startswith(('0x', '-0x')):
            float.fromhex(x)
            return True
        return x.replace('_', '').replace(' ', '').replace('/', '').isalnum()          # names: mesh, group, format
    return isinstance(x, (bool, int, float))


def test_files_are_small_and_hold_data_only():
    gen = _generator()
    for name, doc in ec.documents().items():
        assert os.path.getsize(os.path.join(ec.GOLDEN, name + '.gz')) < len(gen.dumps(doc).encode()) < 150*1024, name
        assert _data_only(doc), name


def oracle_results(case):
    """{result: {field: array}} of the numpy oracle"""
    orc = make_oracle_generic(case.mesh, case.bath, **case.oracle_kwargs())
    out = {}
    if case.is_tracer:
        kw = case.tracer_kwargs()
        out['tendency'] = {'tracer': orc.tracer_tendency(case.T, case.uv, case.eta, case.dt, **kw)}
        out['step'] = {'tracer': orc.tracer_ssprk33_step(case.T, case.uv, case.eta, case.dt, **kw)}
        return out
    ku, ke = orc.tendency(case.uv, case.eta, case.dt)
    out['tendency'] = {'uv': ku, 'eta': ke}
    u, e = orc.ssprk33_step(case.uv, case.eta, case.dt)
    out['step'] = {'uv': u, 'eta': e}
    if 'two_steps' in case.exact:
        u, e = orc.ssprk33_step(u, e, case.dt)
        out['two_steps'] = {'uv': u, 'eta': e}
    return out


def ref_results(case, ref_so):
    """{result: {field: array}} of the C restatement"""
    mesh = case.mesh
    ref = ref_so.RefSWE(mesh.cell_xy(), mesh.cell_nbr, mesh.cell_nbr_facet, case.bath[mesh.cells], boundary_len=mesh.boundary_len,
                        **case.ref_kwargs())
    if case.is_tracer:
        tr = ref_so.RefTracer(ref, **case.ref_tracer_kwargs())
        return {'tendency': {'tracer': tr.tendency(case.T, case.uv, case.dt)}, 'step': {'tracer': tr.step(case.T, case.uv, case.dt)}}
    ku, ke = ref.tendency(case.uv, case.eta, case.dt)
    out = {'tendency': {'uv': ku, 'eta': ke}}
    u, e = ref.advance(case.uv, case.eta, case.dt, 1)
    out['step'] = {'uv': u, 'eta': e}
    if 'two_steps' in case.exact:
        u, e = ref.advance(case.uv, case.eta, case.dt, 2)
        out['two_steps'] = {'uv': u, 'eta': e}
    return out


def _check(case, results, what):
    worst = 0.0
    for res, fields in results.items():
        for f, val in fields.items():
            err = ec.rel_err(val, case.exact[res][f])
            print('{:} {:} {:}.{:}: rel_linf {:.2e} = {:.2f} eps*max|exact|'.format(
                case.name, what, res, f, err, ec.eps_units(val, case.exact[res][f])))
            worst = max(worst, err)
            assert err < TOL, (case.name, what, res, f, err)
    return worst


@pytest.mark.parametrize('name', NAMES)
def test_numpy_oracle_matches_exact_weak_forms(name):
    case = ec.cases()[name]
    results = oracle_results(case)
    assert set(results) == set(case.exact)
    _check(case, results, 'numpy oracle')


# the cases the C restatement has every option of; which they must be is written down in test_c_restatement_covers_what_it_can_express
C_NAMES = [n for n in NAMES if ec.cases()[n].ref_expected()]


@pytest.mark.parametrize('name', C_NAMES)
def test_c_restatement_matches_exact_weak_forms(ref_so, name):
    case = ec.cases()[name]
    results = ref_results(case, ref_so)
    assert set(results) == set(case.exact)
    _check(case, results, 'C restatement')


def test_c_restatement_covers_what_it_can_express():
    """by name, on both small meshes: walls, the seven boundary kinds and all four markers with constant data, every source alone
    (the drag as a constant), the advection-only tracer cases; and both 72-cell cases with sources (one and two steps)"""
    small = (['walls', 'bnd_all_four_constant', 'src_linear_drag_constant', 'tracer_advection', 'tracer_advection_lf']
             + ['bnd_' + '_'.join(kind) for kind in ec.BND_KINDS]
             + ['src_' + key for key in ec.SOURCES if key != 'linear_drag'])
    expected = {m + '/' + n for m in ('tri8', 'quad4') for n in small} | {'tri345/all_four_coriolis_drag', 'quad72/all_four_coriolis_drag'}
    assert set(C_NAMES) == expected, set(C_NAMES) ^ expected
    for name in ('tri345/all_four_coriolis_drag', 'quad72/all_four_coriolis_drag'):
        assert 'two_steps' in ec.cases()[name].exact and ec.cases()[name].mesh.num_cells == 72


def test_every_case_carries_its_feature():
    for name, case in ec.cases().items():
        assert case.share >= 1e-3, (name, case.share)


def test_cases_reach_every_boundary_kind_and_source_on_both_cell_types():
    n = collections.Counter()
    for case in ec.cases().values():
        k = case.mesh.cells.shape[1]
        for kind, how in case.kinds():
            n[k, kind] += 1
            n[k, kind[0] if len(kind) == 1 else None, how] += 1
        for key, v in case.raw.get('sources', {}).items():
            n[k, key] += 1
            n[k, key, 'field' if np.ndim(v) else 'const'] += 1
        if 'viscosity' in case.raw:
            v = case.raw['viscosity']
            n[k, 'visc', 'field' if np.ndim(v['nu']) else 'const'] += 1
            n[k, 'visc', np.ndim(v['nu']) > 0, v['grad_div'], v['sipg_factor']] += 1
        if case.is_tracer:
            t = case.raw['tracer']
            n[k, 'tracer', t['conservative'], t['lax_friedrichs']] += 1
            if 'diffusivity' in t:
                n[k, 'mu', 'field' if np.ndim(t['diffusivity']) else 'const'] += 1
        n[k, 'cells', case.mesh.num_cells] += 1
        n[k, 'two_steps'] += 'two_steps' in case.exact
    for k in (3, 4):
        for kind in ec.BND_KINDS:
            assert n[k, kind] >= 1, (k, kind)
        for key in ('elev', 'uv', 'un', 'flux'):
            assert n[k, key, 'const'] >= 1 and n[k, key, 'field'] >= 1, (k, key)
        for key in ec.SOURCES:
            assert n[k, key] >= 2, (k, key)               # alone and together
        assert n[k, 'linear_drag', 'const'] >= 1 and n[k, 'linear_drag', 'field'] >= 1
        for key in [('mu', 'field'), ('mu', 'const')] + [('visc', f, gd, sf) for f in (False, True) for gd in (False, True)
                                                         for sf in (1.0, 2.0)]:
            assert n[(k,) + key] >= 1, (k, key)
        for cons in (True, False):
            for lf in (True, False):
                assert n[k, 'tracer', cons, lf] >= 1
        assert n[k, 'cells', 72] >= 1 and n[k, 'two_steps'] >= 1


def error_table(ref_so):
    """per case: inf-norm error of the numpy oracle and of the C restatement in units of eps*max|exact| (tendency / step)"""
    lines = ['# error against the exactly integrated weak forms in units of eps*max|exact| (eps = 2^-52); worst field of the case',
             '# {:<44s} {:>10s} {:>10s} {:>10s} {:>10s} {:>9s}'.format('case', 'numpy tend', 'numpy step', 'C tend', 'C step', 'share')]
    for name in NAMES:
        case = ec.cases()[name]
        row = []
        for results in (oracle_results(case), ref_results(case, ref_so) if case.ref_expected() else None):
            for res in ('tendency', 'two_steps' if 'two_steps' in case.exact else 'step'):
                row.append('n/a' if results is None else '{:.2f}'.format(
                    max(ec.eps_units(v, case.exact[res][f]) for f, v in results[res].items())))
        lines.append('{:<46s} {:>10s} {:>10s} {:>10s} {:>10s} {:>9.2e}'.format(name, *row, case.share))
    lines.append('# step: after one SSPRK33 step (after two on the 72-cell meshes); n/a: the C restatement has no such option')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    from oracle import ref_lib
    ref_lib.build()
    with open(sys.argv[1], 'w') as fh:
        fh.write(error_table(ref_lib))
