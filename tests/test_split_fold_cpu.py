"""Host fold of a filter into a split plane's two-step test (DESIGN.md §9h;
tikv_amd/csrc/plane_fold.h split_fc_fold / split_row_in).

Compiles tests/split_fold_main.cpp, a stand-alone program with its own main,
with the host compiler and -fsanitize=address,undefined and runs it
directly. The program checks split_fc_fold + split_row_in against the 32-bit
narrow test and that against the 64-bit reference and a direct comparison:
six comparers, both signednesses, NULL and non-NULL constants, planes with
nmax in {0x10000, 0x1FFFF, 0x30000, 0xFFFFFFFF} at bases {INT64_MIN, -3, 0,
INT64_MAX - 0xFFFFFFFF}, constants that put the folded bounds on the low
halves 0x0000, 0x0001, 0xFFFE and 0xFFFF, equal high halves, empty and full
intersections; stored values +-2 around both bounds and around every
multiple of 65536 next to them, 0 and nmax; and the interval property: no
row inside the sure interval fails the full test, none outside the maybe
interval passes it.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def test_split_fold_matches_narrow_and_wide_reference(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "split_fold_check")
    src = os.path.join(HERE, "split_fold_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "0 mismatches" in run.stdout, run.stdout
