"""The staging-slot sources of the two-ring tiles (thetis_amd/csrc/swe2d_tiles.h: slot_src, slot_first), on the host.

The three-stage kernel gathers the traces from outside a tile slot by slot: lane s loads the six values the table names for slot s.
tests/tile_slots_main.cpp, a program of its own compiled with the address and undefined-behaviour sanitizers (nothing is loaded into
this interpreter), builds the tables of the meshes of tests/test_gpu_fuse3_slots.py and checks that every slot named in a lane's facet
field has exactly one source, that the source is the neighbour the connectivity names, and that no tile has more than
SWE_FUSE3_MAX_OUT = 224 slots."""
import os
import re
import shutil
import subprocess

import pytest

import slot_cases
import tile_cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('tile_slots')/'tile_slots_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'tile_slots_main.cpp'), '-o', exe])
    return exe


def _run(program, tmp_path, case):
    inp = str(tmp_path/'in.bin')
    tile_cases.write_builder_input(inp, case, 'triple')
    r = subprocess.run([program, inp], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr)             # (a sanitizer report goes to stderr)
    m = re.fullmatch(r'tiles (\d+) max_slots (\d+) total (\d+)\n', r.stdout)
    assert m, r.stdout
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize('name', slot_cases.NAMES)
def test_every_slot_has_one_source_and_it_is_the_neighbour(program, tmp_path, name):
    tiles, max_slots, total = _run(program, tmp_path, slot_cases.builder_case(name))
    assert max_slots <= 224
    if name == 'tri3x2':
        assert (tiles, max_slots, total) == (1, 0, 0)       # one tile holds the mesh: nothing outside it
    elif name == 'tri23x17_patches11x8':
        assert tiles == 9 and 0 < max_slots and total > 0   # 3 x 3 patches, the last row and column ragged
    elif name == 'tri23x17_patches5x3':
        assert tiles == 30 and 0 < max_slots
    else:
        assert tiles > 8 and max_slots > 128                # more slots than the lanes of two waves


def test_the_golden_tile_cases_too(program, tmp_path):
    """the meshes of tests/golden/tile_tables.json: partitions, the coast mesh, the library's own runs"""
    for name, c in tile_cases.cases().items():
        if 'triple' in c['kinds']:
            tiles, max_slots, _ = _run(program, tmp_path, c)
            assert tiles >= 3 and max_slots <= 224, name
