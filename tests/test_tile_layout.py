"""The third plane of the lane records and the plane layout of the staging area of the three-stage kernel (thetis_amd/csrc/swe2d_tiles.h:
LaneRecords::lane_slot, kStagingPlanes), on the host.

A lane of a tile used to find the staging slot it gathers through two per-tile arrays - {first, count} of the tile, then the slot's two
byte offsets - and wrote the six values to [slot][6].  Now the offsets lie in a third plane of its record, by physical lane, with a
sentinel for a lane without a slot, and the six values go to index `lane` of six planes of P1, so that an outside trace is addressed
like an inside one.  tests/tile_layout_main.cpp, a program of its own compiled with the address and undefined-behaviour sanitizers
(nothing is loaded into this interpreter), builds the records in both layouts and checks the plane against the old arrays under the
slot -> lane map, the sentinel, every outside trace word against the plane and index its slot's writer fills (inside P1), and that
the inside words are unchanged.

Cases: the meshes of tests/slot_cases.py and the two-ring cases of tests/golden/tile_tables.json (tests/tile_cases.py), and the tree of
tests/test_tile_records.py, whose first tile has the maximum of 224 slots.  'tri3x2' is one tile without a slot and 244 padding lanes;
'tri23x17_patches11x8' has nine tiles with all four rotations; every mesh here has padding lanes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import slot_cases
import tile_cases
from test_tile_records import _device_cells, _planes, _tree

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ('tiles', 'real', 'padding', 'rotations', 'max_slots', 'min_slots', 'slots', 'outside')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('tile_layout')/'tile_layout_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tile_layout_main.cpp'), '-o', exe])
    return exe


def _run(program, tmp_path, case, cv, plane_bytes=None):
    """cv: [n][3] vertex ids in the numbering of the case's cells"""
    inp = str(tmp_path/'in.bin')
    tile_cases.write_builder_input(inp, case, 'triple')
    stride = case['codes'].shape[1]
    with open(inp, 'ab') as f:
        _planes(cv, stride).tofile(f)
        np.array([8*stride if plane_bytes is None else plane_bytes], dtype=np.int32).tofile(f)
    r = subprocess.run([program, inp], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr)             # (a sanitizer report goes to stderr)
    m = re.fullmatch(' '.join(k + r' (\d+)' for k in FIELDS) + '\n', r.stdout)
    assert m, r.stdout
    out = dict(zip(FIELDS, (int(x) for x in m.groups())))
    assert out['real'] + out['padding'] == 256*out['tiles'] and out['outside'] == out['slots']
    return out


@pytest.mark.parametrize('name', slot_cases.NAMES)
def test_slot_plane_and_plane_layout(program, tmp_path, name):
    case = slot_cases.builder_case(name)
    out = _run(program, tmp_path, case, _device_cells(case))
    assert out['padding'] > 0
    if name == 'tri3x2':
        assert (out['tiles'], out['real'], out['slots'], out['max_slots']) == (1, 12, 0, 0)          # a tile with no slot
    elif name == 'tri23x17_patches11x8':
        assert out['tiles'] == 9 and out['rotations'] == 0b1111 and out['slots'] > 0
    elif name == 'tri23x17_patches5x3':
        assert out['tiles'] == 30 and out['rotations'] == 0b1111
    else:
        assert out['tiles'] > 8 and out['max_slots'] > 128 and out['rotations'] == 0b1111


def test_the_golden_tile_cases_too(program, tmp_path):
    """the two-ring cases of tests/golden/tile_tables.json, a partition among them, with a state plane longer than the connectivity
    planes (the slot offsets are multiples of that length)"""
    seen = 0
    for name, c in tile_cases.cases().items():
        if 'triple' in c['kinds']:
            n = c['nbr'].shape[0]
            out = _run(program, tmp_path, c, np.asarray(c['mesh'].cells)[:n], plane_bytes=8*(c['codes'].shape[1] + 192))
            assert out['tiles'] >= 3, name
            seen += 1
    assert seen > 0


def test_a_tile_with_the_maximum_of_224_slots(program, tmp_path):
    """56 lanes of every wave gather a slot: the writers' indices reach 64*3 + 55 = 247, inside the 256 of a plane"""
    nb, nbf = _tree(8)
    case = {'codes': tile_cases.packed_codes(nb, nbf), 'nbr': nb, 'order': None, 'triple_order': None, 'triple_start': None}
    cv = np.random.default_rng(5).integers(0, 2**17, size=nb.shape)
    out = _run(program, tmp_path, case, cv)
    assert out['max_slots'] == 224 and out['padding'] > 0, out
