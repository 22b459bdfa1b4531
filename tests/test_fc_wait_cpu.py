"""The host end of the filter+count hand-over (DESIGN.md §9n;
tikv_amd/csrc/fc_wait.h wait_seq and ticks_to_ns).

Compiles tests/fc_wait_main.cpp, a stand-alone program with its own main,
with the host compiler and runs it directly: once with
-fsanitize=address,undefined and, where the toolchain links it, once with
-fsanitize=thread. In the program a std::thread plays the device: it stores
count and ticks, then the sequence number with release ordering. Checked:
arrival with both words visible for 4000 consecutive numbers; a stale number
(one less than expected, stored once or over and over) and a writer that never
comes give "expired", never earlier than the deadline and, in the shortest of
nine runs, within two batches of spins and 16 clock steps of it, both timed
in the program; deadline 0 gives "expired" even when the word is there; ticks_to_ns
against 128-bit integer arithmetic for 0, 1, 2^63 / rate and their neighbours
at 100 MHz, 1 kHz and other rates, saturating past 64 bits.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "fc_wait_main.cpp")


def _host_compiler():
    for cc in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def _build(cxx, exe, sanitize, src=SRC):
    return subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread",
         "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
         src, "-o", exe],
        capture_output=True, text=True)


# the smallest program that needs ThreadSanitizer's runtime and a second thread
TRIVIAL = """#include <thread>
int main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }
"""


def _run(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert ", 0 mismatches" in run.stdout, run.stdout


def test_wait_and_ticks_address_undefined(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fc_wait_check")
    cc = _build(cxx, exe, "address,undefined")
    assert cc.returncode == 0, cc.stderr[-4000:]
    _run(exe)


def test_wait_thread_sanitizer(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # whether the toolchain links -fsanitize=thread and its runtime starts
    # here is asked of a trivial program; the real one then runs with no skip
    trivial = tmp_path / "trivial.cpp"
    trivial.write_text(TRIVIAL)
    probe_exe = str(tmp_path / "trivial")
    if _build(cxx, probe_exe, "thread", str(trivial)).returncode != 0:
        pytest.skip("this toolchain does not link -fsanitize=thread")
    if subprocess.run([probe_exe], capture_output=True).returncode != 0:
        pytest.skip("ThreadSanitizer's runtime does not start here")
    exe = str(tmp_path / "fc_wait_check")
    cc = _build(cxx, exe, "thread")
    assert cc.returncode == 0, cc.stderr[-4000:]
    _run(exe)
