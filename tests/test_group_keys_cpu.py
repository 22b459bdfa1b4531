"""Tuple dictionary of multi-key hash aggregation (DESIGN.md §9j;
tikv_amd/csrc/group_keys.h), the header the device kernels and the host both
include.

Compiles tests/group_keys_main.cpp, a stand-alone program with its own main,
with the host compiler and -fsanitize=address,undefined and runs it directly.
The program checks the slot word's pack / unpack round trip (rep_row =
2^32 - 2 included), tuple equality with NULL against 0, and a sequential
insert / lookup model of the probe loop over small tables against std::map:
wrap-around past the last slot, the full flag, and that equal fingerprints
with different tuples land in different slots.
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


def test_group_key_dictionary_model(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "group_keys_check")
    src = os.path.join(HERE, "group_keys_main.cpp")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert ", 0 mismatches" in run.stdout, run.stdout
