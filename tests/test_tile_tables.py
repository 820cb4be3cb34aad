"""thetis_amd/csrc/swe2d_tiles.h, the tile-table builder of the fused stage kernels, by itself on the host.

tests/tile_tables_main.cpp is compiled with the address and undefined-behaviour sanitizers and run as a child process per case (nothing
is loaded into this interpreter).  Its tables must be, packed as swe2d_api_fuse.hip packs them, byte for byte those in
tests/golden/tile_tables.json - digests written once from the three builder loops the single one replaced - and must say what the
kernels rely on: each cell interior in exactly one tile, every facet field the lane that holds the neighbour, the rings complete."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tile_cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, 'golden', 'tile_tables.json')))
CAPS = {'pair': (1, 192, 64, 128), 'quad': (1, 192, 64, 192), 'triple': (2, 256, 256, 224)}       # rings, interior, ring 1, staging slots
KEYS = sorted(GOLDEN)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('tile_tables')/'tile_tables_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tile_tables_main.cpp'), '-o', exe])
    return exe


def _run(program, tmp_path, c, kind):
    inp, out = str(tmp_path/'in.bin'), str(tmp_path/'out.bin')
    tile_cases.write_builder_input(inp, c, kind)
    r = subprocess.run([program, kind, inp, out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr)             # (a sanitizer report goes to stderr)
    a = np.fromfile(out, dtype=np.int32)
    n_tiles, wg, nf, ring1, ring2 = (int(x) for x in a[:5])
    t, o = {'n_tiles': n_tiles, 'wg': wg, 'ring': [ring1, ring2]}, 5
    for key, size in (('cell', n_tiles*wg), ('facet', n_tiles*wg*nf), ('n_inner', n_tiles), ('n_mid', n_tiles), ('rot', n_tiles)):
        t[key] = a[o:o + size]
        o += size
    assert o == len(a)
    t['facet'] = t['facet'].reshape(-1, nf)
    return t


def test_the_cases_are_the_golden_ones():
    assert KEYS == sorted(name + ':' + kind for name, c in tile_cases.cases().items() for kind in c['kinds'])


@pytest.mark.parametrize('key', KEYS)
def test_tables_are_those_of_the_three_builders_they_replace(program, tmp_path, key):
    name, kind = key.split(':')
    t = _run(program, tmp_path, tile_cases.cases()[name], kind)
    gold = GOLDEN[key]
    assert (t['n_tiles'], t['ring']) == (gold['n_tiles'], gold['ring'])
    assert t['n_tiles'] >= 3
    assert hashlib.sha256(tile_cases.device_stream(kind, t).tobytes()).hexdigest() == gold['sha256']


@pytest.mark.parametrize('key', KEYS)
def test_tables_say_what_the_kernels_rely_on(program, tmp_path, key):
    name, kind = key.split(':')
    c = tile_cases.cases()[name]
    nbr = c['nbr']                                          # [n][facets] neighbour or -marker, device numbering
    n, nf = nbr.shape
    order, start = tile_cases.builder_input(c, kind)
    order = np.arange(n) if order is None else order
    rings, max_inner, max_ring1, max_out = CAPS[kind]
    t = _run(program, tmp_path, c, kind)
    wg = t['wg']
    assert wg == 256
    interior_of = np.full(n, -1)
    pos = 0
    ring_cells = [0, 0]
    for tile in range(t['n_tiles']):
        cell = t['cell'][tile*wg:(tile + 1)*wg]
        facet = t['facet'][tile*wg:(tile + 1)*wg]
        ni, nm, rot = int(t['n_inner'][tile]), int(t['n_mid'][tile]), int(t['rot'][tile])
        assert rot == (tile_cases.rot_of_tile(tile) if kind == 'triple' else 0)
        role = (np.arange(wg) - 64*rot) % wg               # of the physical lanes
        nt = int((cell >= 0).sum())
        assert 1 <= ni <= nm <= nt <= 256 and ni <= max_inner and nm - ni <= max_ring1
        assert nm == nt if rings == 1 else (nt - nm)*2 <= max_out
        assert ((cell >= 0) == (role < nt)).all()           # roles [interior | ring 1 | ring 2 | padding], nothing in between
        assert (facet[cell < 0] == 0).all()
        lane_of = {int(cl): l for l, cl in enumerate(cell) if cl >= 0}
        assert len(lane_of) == nt                           # no cell twice in a tile
        by_role = cell[np.argsort(role)]
        inner, ring1, ring2 = by_role[:ni], by_role[ni:nm], by_role[nm:nt]
        # the interior: the next cells of the order, each in exactly one tile; the caller's starts begin a tile
        assert (inner == order[pos:pos + ni]).all()
        assert (interior_of[inner] == -1).all()
        interior_of[inner] = tile
        if start is not None:
            assert not start[pos + 1:pos + ni].any()
        pos += ni

        def facet_neighbours(cells):
            nb = nbr[cells].ravel()
            return set(int(x) for x in nb[nb >= 0])
        assert set(int(x) for x in ring1) == facet_neighbours(inner) - set(int(x) for x in inner)
        if rings == 2:
            assert set(int(x) for x in ring2) == facet_neighbours(ring1) - set(int(x) for x in inner) - set(int(x) for x in ring1)
        ring_cells[0] += nm - ni
        ring_cells[1] += nt - nm
        outermost = nm if rings == 2 else ni                # the first role that may have a neighbour outside the tile
        slots = []
        for l in range(wg):
            if cell[l] < 0:
                continue
            for f in range(nf):
                w, nb = int(facet[l, f]), int(nbr[cell[l], f])
                assert w < 0x400
                if nb < 0:
                    assert w == l                           # a boundary facet names the lane itself
                elif nb in lane_of:
                    assert w == lane_of[nb]
                else:
                    assert w & 0x200 and role[l] >= outermost
                    slots.append(w & 0x1ff)
        assert len(set(slots)) == len(slots) and all(s < max_out for s in slots)
        assert sorted(slots) == list(range(len(slots)))
    assert pos == n and (interior_of >= 0).all()
    assert ring_cells == t['ring']


def test_isolated_cells_and_a_bad_input(program, tmp_path):
    """every facet a boundary: no rings, the two-ring tiles hold 256 interior cells each; an input whose header is wrong is an error
    of the program (status 1), not a read out of bounds"""
    c = dict(tile_cases.cases()['tri24x16'])
    c['codes'] = np.full_like(c['codes'], -1)
    t = _run(program, tmp_path, c, 'triple')
    assert t['n_tiles'] == 3 and t['ring'] == [0, 0] and list(t['n_inner']) == [256, 256, 256]
    inp = str(tmp_path/'bad.bin')
    np.array([3, 10, 768, 0, 0], dtype=np.int32).tofile(inp)
    r = subprocess.run([program, 'triple', inp, str(tmp_path/'out.bin')], capture_output=True, text=True)
    assert r.returncode == 1 and 'bad header' in r.stderr
