"""Host fold of a filter into a split plane's bucket index (DESIGN.md §9q;
tikv_amd/csrc/plane_fold.h bucket_fc_fold).

Compiles tests/bucket_fold_main.cpp, a stand-alone program with its own main,
with the host compiler and -fsanitize=address,undefined and runs it
directly. The program builds, for random columns of 1 to 300 values inside
one bucket, over two adjacent buckets and over wide ranges, the 65 537
offsets and the low halves grouped by bucket, and checks bucket_fc_fold plus
the slice rule (in = sure + the slice rows that pass split_full_in, count =
invert ? n - in : in) against split_row_in row by row, the 64-bit reference
and a direct comparison: six comparers, both signednesses, NULL and non-NULL
constants, constants c - 1, c, c + 1 around every bucket bound and around min
and max, the "never" form, and offsets that are no offsets.
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


def test_bucket_fold_matches_split_rows_and_wide_reference(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "bucket_fold_check")
    src = os.path.join(HERE, "bucket_fold_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "0 mismatches" in run.stdout, run.stdout
