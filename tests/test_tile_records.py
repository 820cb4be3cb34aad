"""The lane records of the three-stage kernel (thetis_amd/csrc/swe2d_tiles.h: build_lane_records), on the host.

The kernel's prologue used to decode, in every lane of every tile of every step, what depends on the mesh and the tile table alone: the
connectivity record, bmarkers, per facet the two LDS byte addresses of the neighbour's traces, per vertex its byte offset, per staging
slot the two byte offsets of its source.  The host now does it once per table.  tests/tile_records_main.cpp, a program of its own
compiled with the address and undefined-behaviour sanitizers (nothing is loaded into this interpreter), builds tables and records and
compares every field of every lane and slot with the restated prologue: swe_conn_pack / swe_conn_unpack or the wide records, then the
prologue's formulas.

Cases: the meshes of tests/slot_cases.py and the two-ring cases of tests/tile_cases.py, and two synthetic ones -
  * 'escape': 262 812 triangles in the mesh's own numbering with two cell labels exchanged, 3 and n - 5, so that cell 3 and its
    neighbours (and cell n - 5 and its) differ by more than 2^18: their 16-B connectivity records are escapes to the wide ones;
  * 'tree': a connectivity that is a tree, every cell with a parent and two children, in breadth-first numbering.  No planar mesh has
    it, and the builder does not care: a tile's interior of 54 cells has a first ring of 56 and a second ring of 112 cells with two
    facets towards the outside each, 224 staging slots - SWE_FUSE3_MAX_OUT, the maximum, where the builder closes the tile.
The rectangles have corner cells with two boundary facets and tiles with padding lanes; 'tri23x17_patches11x8' has nine tiles, whose
rotations are 0, 2, 0, 3, 1, ...: all four."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import slot_cases
import tile_cases

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ('tiles', 'real', 'padding', 'escapes', 'corners', 'rotations', 'max_slots', 'slots')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('tile_records')/'tile_records_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tile_records_main.cpp'), '-o', exe])
    return exe


def _planes(a, stride):
    """[n][3] -> [3][stride] int32"""
    out = np.zeros((3, stride), dtype=np.int32)
    out[:, :a.shape[0]] = np.asarray(a).T
    return out


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
    return dict(zip(FIELDS, (int(x) for x in m.groups())))


def _device_cells(case):
    """the cell vertices in the device numbering of a whole-mesh case"""
    mesh = case['mesh']
    return np.asarray(mesh.cells)[tile_cases.device_numbering(mesh)[0]]


@pytest.mark.parametrize('name', slot_cases.NAMES)
def test_every_field_is_what_the_prologue_formed(program, tmp_path, name):
    case = slot_cases.builder_case(name)
    out = _run(program, tmp_path, case, _device_cells(case))
    assert out['real'] + out['padding'] == 256*out['tiles'] and out['padding'] > 0 and out['escapes'] == 0
    if name == 'tri3x2':
        assert (out['tiles'], out['real'], out['slots'], out['corners']) == (1, 12, 0, 2)
    elif name == 'tri23x17_patches11x8':
        assert out['tiles'] == 9 and out['rotations'] == 0b1111 and out['corners'] >= 2 and out['slots'] > 0
    elif name == 'tri23x17_patches5x3':
        assert out['tiles'] == 30 and out['rotations'] == 0b1111 and out['corners'] >= 2
    else:
        assert out['tiles'] > 8 and out['max_slots'] > 128 and out['rotations'] == 0b1111


def test_the_golden_tile_cases_too(program, tmp_path):
    """the two-ring cases of tests/golden/tile_tables.json, a partition among them (any vertex ids serve: the builder scales them by 8 -
    the caller's numbering of the cells here), with a state plane longer than the connectivity planes"""
    for name, c in tile_cases.cases().items():
        if 'triple' in c['kinds']:
            n = c['nbr'].shape[0]
            out = _run(program, tmp_path, c, np.asarray(c['mesh'].cells)[:n], plane_bytes=8*(c['codes'].shape[1] + 192))
            assert out['tiles'] >= 3 and out['real'] + out['padding'] == 256*out['tiles'], name


def test_escape_connectivity_records(program, tmp_path):
    """cells whose neighbours are 2^18 labels and more away: swe_conn_pack gives an escape, the reference reads the wide records"""
    from thetis_amd.mesh import RectangleMesh
    mesh = RectangleMesh(363, 362, 100e3, 100e3)
    nb, nbf, cells = np.asarray(mesh.cell_nbr).astype(np.int64), np.asarray(mesh.cell_nbr_facet).astype(np.int64), np.asarray(mesh.cells)
    n = nb.shape[0]
    a, b = 3, n - 5
    assert b - a >= 2**18 and -nb.min() < 256
    p = np.arange(n)
    p[a], p[b] = b, a                                        # an involution: label i sits where label p[i] sat
    nb, nbf, cells = nb[p], nbf[p], cells[p]
    nb[nb >= 0] = p[nb[nb >= 0]]
    case = {'codes': tile_cases.packed_codes(nb, nbf), 'nbr': nb, 'order': None, 'triple_order': None, 'triple_start': None}
    out = _run(program, tmp_path, case, cells)
    # cells a and b and their three neighbours each, once as interior cells and again in the rings of the tiles around them
    assert out['escapes'] >= 8 and out['real'] > n and out['corners'] >= 2


def _tree(depth):
    """neighbour codes [n][3] of a tree in breadth-first numbering: facet 0 leads to the parent (the root: to a third child), facets 1
    and 2 to the children, whose facet 0 leads back; the leaves' other facets lie on the boundary, marker 1"""
    n = 1 + 3*(2**depth - 1)
    nb, nbf, level = np.full((n, 3), -1, dtype=np.int64), np.zeros((n, 3), dtype=np.int64), np.zeros(n, dtype=np.int64)
    nxt = 1
    for c in range(n):
        for f in ((0, 1, 2) if c == 0 else (1, 2)):
            if level[c] < depth:
                nb[c, f], nbf[c, f] = nxt, 0
                nb[nxt, 0], nbf[nxt, 0], level[nxt] = c, f, level[c] + 1
                nxt += 1
    assert nxt == n
    return nb, nbf


def test_a_tile_with_the_maximum_of_224_slots(program, tmp_path):
    """the largest the builder can reach IS the maximum: 112 second-ring cells with two facets towards the outside each"""
    nb, nbf = _tree(8)
    case = {'codes': tile_cases.packed_codes(nb, nbf), 'nbr': nb, 'order': None, 'triple_order': None, 'triple_start': None}
    cv = np.random.default_rng(5).integers(0, 2**17, size=nb.shape)      # (differences that fit the 16-B record)
    out = _run(program, tmp_path, case, cv)
    assert out['max_slots'] == 224 and out['corners'] > 0 and out['escapes'] == 0, out
