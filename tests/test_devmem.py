"""The owner type of the library's device memory (thetis_amd/csrc/swe2d_devmem.h: DevArray, swe_dev_alloc / swe_dev_free), on the host.

tests/devmem_main.cpp, a program of its own compiled with the address and undefined-behaviour sanitizers (nothing is loaded into
this interpreter), defines the funnel over malloc / free with live counters and an allocation that fails on demand, and exercises
alloc / ensure / reset, the moves (onto a full target and onto itself too), a std::vector of a struct with three arrays growing past
its capacity, and a build function that fails at its first, second and third allocation.  After every sub-case its live counters are
zero; a leak, a double free or a use after free is the sanitizers' report on stderr."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_devarray_frees_what_it_owns_exactly_once(tmp_path):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path/'devmem_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'devmem_main.cpp'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr)             # (a sanitizer report goes to stderr)
    assert r.stdout == 'ok 6\n', r.stdout


def test_devmem_header_stays_one_screen():
    """the owner type does one thing (no copies, no allocator parameters): about 80 lines at the most, and no HIP include"""
    text = open(os.path.join(HERE, '..', 'thetis_amd', 'csrc', 'swe2d_devmem.h')).read()
    assert len(text.splitlines()) <= 80
    assert '#include <hip' not in text and '#include "hip' not in text
