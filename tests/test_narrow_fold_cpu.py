"""Host fold of a filter into a narrow plane's domain (DESIGN.md §9e;
tikv_amd/csrc/plane_fold.h narrow_fc_fold).

Compiles tests/narrow_fold_main.cpp, a stand-alone program with its own
main, with the host compiler and -fsanitize=address,undefined and runs it
directly. The program brute-forces the 32-bit fold against the 64-bit
reference (plane_fc_fold plus k_plane_fc's row expression) and against a
direct comparison: six comparers, both signednesses, NULL and non-NULL
constants, bases in {INT64_MIN, -3, 0, INT64_MAX - 300}, ranges in
{0, 1, 255, 256, 65535}, every stored value up to a few hundred per case,
constants around each edge of the plane plus the extremes.
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


def test_narrow_fold_matches_wide_reference(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "narrow_fold_check")
    src = os.path.join(HERE, "narrow_fold_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "0 mismatches" in run.stdout, run.stdout
