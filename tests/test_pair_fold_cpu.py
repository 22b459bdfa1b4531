"""plane_fc_and, the host fold of two conditions on one column (DESIGN.md
§9r): builds tests/pair_fold_main.cpp, a stand-alone program whose header says
what it checks, with -fsanitize=address,undefined and runs it directly."""
import os
import subprocess

import pytest

from test_split_fold_cpu import HERE, _host_compiler


def test_pair_fold_matches_the_and_of_both_conditions(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pair_fold_check")
    cc = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(HERE, "pair_fold_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "0 mismatches" in run.stdout, run.stdout
