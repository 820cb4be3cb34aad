"""GPU: the HIP stage kernels against exactly integrated weak forms (tests/golden/exact_weakforms*.json.gz: rational arithmetic from the
reference's UFL text, no rounding, no quadrature, nothing shared with the oracle; tests/golden/make_exact_weakform_golden.py).

Bounds are the suite's own, now against values without rounding: tendency rel_linf < TOL = 2e-12, a step (three ``solve_stage``
calls, and ``advance(1)``) and two steps < 10*TOL (tests/test_gpu_fuzz.py).  On the 72-cell meshes the same exact steps for the stage
launches, the forced fused pair, the forced three-stage kernel and the dataflow kernel, with ``fused_*_info()`` asserting the path.
``python tests/test_gpu_exact_weakforms.py FILE`` writes the table of measured errors to FILE."""
import os
import sys

import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exact_cases as ec
from thetis_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 2e-12
NAMES = sorted(ec.cases())
BIG = [n for n in NAMES if ec.cases()[n].mesh.num_cells >= 64]
PATHS = {'stages': 0, 'pair': 1, 'triple': 3}


def _errors(case, res, got):
    """{field: (rel_linf, error in eps*max|exact|)}"""
    return {f: (ec.rel_err(v, case.exact[res][f]), ec.eps_units(v, case.exact[res][f])) for f, v in got.items()}


def _assert(case, res, got, bound, what, log=None):
    errs = _errors(case, res, got)
    for f, (rel, units) in errs.items():
        print('{:} {:} {:}.{:}: rel_linf {:.2e} = {:.2f} eps*max|exact|'.format(case.name, what, res, f, rel, units))
    if log is not None:
        log[res] = max(u for _, u in errs.values())
    for f, (rel, _) in errs.items():
        assert rel < bound, (case.name, what, res, f, rel)


def _state(dev):
    u, e = dev.get_state()
    return {'uv': u, 'eta': e}


def measure(case, reorder='auto', log=None):
    """tendency, three solve_stage calls, advance(1) (and a second step where the file has one) against the exact values"""
    dev = case.make_device(reorder)
    try:
        if case.is_tracer:
            tid = case.add_device_tracer(dev)
            _assert(case, 'tendency', {'tracer': dev.tracer_tendency(tid)}, TOL, 'kernel', log)
            for s in range(3):
                dev.tracer_solve_stage(tid, s)
            _assert(case, 'step', {'tracer': dev.tracer_get_state(tid)}, 10*TOL, 'kernel', log)
            return
        ku, ke = dev.tendency()
        _assert(case, 'tendency', {'uv': ku, 'eta': ke}, TOL, 'kernel', log)
        for s in range(3):
            dev.solve_stage(s)
        _assert(case, 'step', _state(dev), 10*TOL, 'solve_stage x 3', log)
        dev.set_state(case.uv, case.eta)
        dev.advance(1)
        _assert(case, 'step', _state(dev), 10*TOL, 'advance(1)')
        if 'two_steps' in case.exact:
            dev.advance(1)
            _assert(case, 'two_steps', _state(dev), 10*TOL, 'advance(1) x 2', log)
    finally:
        dev.close()


@pytest.mark.parametrize('name', NAMES)
def test_kernels_match_exact_weak_forms(hip_lib, name):
    measure(ec.cases()[name], reorder=('hilbert' if NAMES.index(name) % 2 else 'auto'))


def _forced(case, path, reorder):
    dev = case.make_device(reorder)
    dev.set_option(_lib.OPT_FLOW, 0)
    dev.set_option(_lib.OPT_FUSED_STAGES, PATHS[path])
    return dev


def _assert_path(dev, path, what):
    """72 cells are one tile without a ring (a tile holds up to 192 interior cells), so what can be asserted is the path itself; tiles
    >= 3 with rings are tests/test_gpu_fuzz_paths.py's, on meshes of 750 cells"""
    if path == 'pair':
        on, tiles, _, cells = dev.fused_pair_info()
        assert on and tiles >= 1, ('the fused stage pair is off', on, tiles, cells, what)
    elif path == 'triple':
        on, tiles, _, _ = dev.fused_triple_info()
        assert on and tiles >= 1, ('the three-stage kernel is off', on, tiles, what)
    else:
        assert not dev.fused_pair_info()[0] and not dev.fused_triple_info()[0], ('a fused kernel is on where stage launches were asked for', what)


# stage launches and the forced pair on both 72-cell meshes; the forced three-stage kernel on the triangle case without source terms
# (the plan keeps it off sources unless forced, and there is no such kernel for quadrilaterals)
PATH_CASES = [(n, p) for n in BIG for p in PATHS
              if p != 'triple' or (ec.cases()[n].mesh.cells.shape[1] == 3 and 'sources' not in ec.cases()[n].raw)]


@pytest.mark.parametrize('reorder', ['auto', 'hilbert'])
@pytest.mark.parametrize('name,path', PATH_CASES)
def test_stepping_paths_match_exact_steps(hip_lib, name, path, reorder):
    case = ec.cases()[name]
    dev = _forced(case, path, reorder)
    try:
        _assert_path(dev, path, (name, reorder))
        dev.advance(1)
        _assert_path(dev, path, (name, reorder))
        _assert(case, 'step', _state(dev), 10*TOL, path)
        if 'two_steps' in case.exact:
            dev.advance(1)
            _assert(case, 'two_steps', _state(dev), 10*TOL, path)
    finally:
        dev.close()


@pytest.mark.parametrize('reorder', ['auto', 'hilbert'])
def test_dataflow_kernel_matches_exact_two_steps(hip_lib, reorder):
    case = ec.cases()['tri345/all_four_coriolis_drag']
    dev = case.make_device(reorder)
    try:
        assert dev.flow_supported(), 'the dataflow kernel declines 72 triangles with Coriolis and linear drag'
        dev.solve_flow([case.mesh.num_cells]*6)
        assert dev.flow_timeouts() == 0
        _assert(case, 'two_steps', _state(dev), 10*TOL, 'solve_flow')
    finally:
        dev.close()


def error_table():
    lines = ['# kernel error against the exactly integrated weak forms in units of eps*max|exact| (eps = 2^-52); worst field of the case',
             '# {:<44s} {:>10s} {:>10s} {:>10s}'.format('case', 'tendency', 'step', 'two steps')]
    for name in NAMES:
        log = {}
        measure(ec.cases()[name], log=log)
        lines.append('{:<46s} {:>10.2f} {:>10.2f} {:>10s}'.format(
            name, log['tendency'], log['step'], '{:.2f}'.format(log['two_steps']) if 'two_steps' in log else '-'))
    lines.append('# the numpy oracle and the C restatement on the same cases: profiles/r13a_exact_weakforms_cpu.txt')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    with open(sys.argv[1], 'w') as fh:
        fh.write(error_table())
