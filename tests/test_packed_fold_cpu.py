"""The packed 16-bit interval count of the filter+count kernels (DESIGN.md
§9l; tikv_amd/csrc/plane_fold.h fold_packed_out and the packed fields of
SplitFcArgs).

Compiles tests/packed_fold_main.cpp, a stand-alone program with its own main,
with the host compiler and -fsanitize=address,undefined and runs it directly.
The program folds narrow tests [a, b] with a and b from {0, 1, 0xFFFF,
0x10000, 0x10001, 0x7FFF0000, 0xFFFEFFFF, 0xFFFF0000, 0xFFFFFFFF} and a seeded
random set, both invert values, the "never" form and all_lo, and for every
pair of halves from {0, 0xFFFF, both ends of both intervals +-1} checks the
packed count of a word against !split_maybe and !split_sure of its two halves,
sure_empty against the 32-bit empty form {0x10000, 0}, and the open-lane rule:
the two counts differ exactly when a half is maybe and not sure.
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


def test_packed_count_matches_per_row_tests(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "packed_fold_check")
    src = os.path.join(HERE, "packed_fold_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "0 mismatches" in run.stdout, run.stdout
