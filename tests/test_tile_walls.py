"""TileSpec::group_walls of the tile-table builder (thetis_amd/csrc/swe2d_tiles.h): the wall cells of a tile on consecutive roles.

A wave of the three-stage kernel with a wall cell among its lanes runs the boundary pass of swe_tri_finish, in every stage that is
active on it; the builder orders the roles inside interior, ring 1 and ring 2 so that as few waves as possible do.  Only the order
inside a class may change: tests/tile_walls_main.cpp, a program of its own compiled with the address and undefined-behaviour sanitizers
(nothing is loaded into this interpreter), builds the tables with and without the grouping and checks that every class is a permutation
of what it was, every trace word and slot still names the same cell and node, the wall cells are consecutive, a tile without a wall
cell keeps its roles and no tile has more (wave, stage) pairs with a wall cell than before.

Meshes: the 23 x 17-quad rectangle in patches of 11 x 8 (corner, edge and ragged patches: nine tiles, all four rotations) and of 5 x 3,
and the tree of tests/test_tile_records.py, whose first tile has the maximum of 224 staging slots and only wall cells in its second ring."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import slot_cases
import tile_cases

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ('tiles', 'wall_tiles', 'moved', 'pairs_before', 'pairs_after', 'max_slots')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('tile_walls')/'tile_walls_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tile_walls_main.cpp'), '-o', exe])
    return exe


def _run(program, tmp_path, case, cv):
    inp = str(tmp_path/'in.bin')
    tile_cases.write_builder_input(inp, case, 'triple')
    stride = case['codes'].shape[1]
    planes = np.zeros((3, stride), dtype=np.int32)
    planes[:, :cv.shape[0]] = np.asarray(cv).T
    with open(inp, 'ab') as f:
        planes.tofile(f)
        np.array([8*stride], dtype=np.int32).tofile(f)
    r = subprocess.run([program, inp], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr)             # (a sanitizer report goes to stderr)
    m = re.fullmatch(' '.join(k + r' (\d+)' for k in FIELDS) + '\n', r.stdout)
    assert m, r.stdout
    out = dict(zip(FIELDS, (int(x) for x in m.groups())))
    print(case.get('name', ''), out)
    return out


@pytest.mark.parametrize('name', ['tri23x17_patches11x8', 'tri23x17_patches5x3'])
def test_rectangle_with_corner_edge_and_ragged_patches(program, tmp_path, name):
    case = slot_cases.builder_case(name)
    mesh = case['mesh']
    out = _run(program, tmp_path, case, np.asarray(mesh.cells)[tile_cases.device_numbering(mesh)[0]])
    if name == 'tri23x17_patches11x8':
        # every one of the nine tiles reaches a wall with one of its rings; their wall cells were spread over the waves
        assert out['tiles'] == 9 and out['wall_tiles'] == 9 and out['moved'] > 0
        assert out['pairs_after'] < out['pairs_before'], out
    else:
        assert out['tiles'] == 30 and out['wall_tiles'] > 0 and out['pairs_after'] <= out['pairs_before'], out


def _tree(depth):
    """neighbour codes of a tree in breadth-first numbering (tests/test_tile_records.py): the leaves' two other facets are walls"""
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
    nb, nbf = _tree(8)
    case = {'codes': tile_cases.packed_codes(nb, nbf), 'nbr': nb, 'order': None, 'triple_order': None, 'triple_start': None}
    cv = np.random.default_rng(5).integers(0, 2**17, size=nb.shape)
    out = _run(program, tmp_path, case, cv)
    assert out['max_slots'] == 224 and out['wall_tiles'] > 0 and out['pairs_after'] <= out['pairs_before'], out
