"""Order-key transform and candidate cut of the multi-key TopN pipeline
(tikv_amd/csrc/topn_keys.h), the header the device kernels
and the host both include.

Compiles tests/topn_keys_main.cpp, a stand-alone program with its own main,
with the host compiler and -fsanitize=address,undefined and runs it directly.
The program brute-forces (value, NULL, unsigned, desc) -> (rank, u) against
the oracle's per-key comparator over the int64/uint64 extremes plus a few
hundred pseudo-random values, both signednesses, both directions and NULL;
checks the inverse transform; and checks the cut rule (sorted composites +
take -> candidate count) against a linear scan, including take > m,
take == m, all-equal and all-distinct arrays.
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


def test_topn_key_transform_and_cut(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "topn_keys_check")
    src = os.path.join(HERE, "topn_keys_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert ", 0 mismatches" in run.stdout, run.stdout
