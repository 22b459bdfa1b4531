"""The IN list over a split plane (tikv_amd/csrc/in_set.h):
builds tests/in_split_main.cpp, a stand-alone program that checks
in_split_fold and in_split_row against std::set of exact integers, with the
host compiler and -fsanitize=address,undefined and runs it directly."""
import os
import subprocess

import pytest

from test_narrow_fold_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))


def test_in_split_matches_exact_integers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "in_split_check")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "in_split_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert ", 0 mismatches" in run.stdout, run.stdout
