"""bench.py command line: a plain run times its steps and nothing else,
--full adds the gates/baselines/secondary lines, --dump-outputs saves the
last timed step's response as float .npy files.

CPU tests cover the dump writer and the option surface; the GPU test runs
one small plain benchmark and checks the dumped count against the oracle."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"],
                       capture_output=True, text=True)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 2


def test_dump_outputs_cfg2(tmp_path):
    bench = _load("bench", BENCH)
    cnt = 10_000_123
    data = bytes([3]) + (cnt ^ (1 << 63)).to_bytes(8, "big")
    assert bench.parse_count(data) == cnt
    d = str(tmp_path / "out")
    bench.dump_outputs(d, "cfg2", cnt, data, 1)
    assert sorted(os.listdir(d)) == ["count.npy", "n_rows.npy",
                                     "response_bytes.npy"]
    resp = np.load(os.path.join(d, "response_bytes.npy"))
    assert resp.dtype == np.float32
    assert bytes(resp.astype(np.uint8)) == data
    c = np.load(os.path.join(d, "count.npy"))
    assert c.dtype == np.float64 and int(c[0]) == cnt
    assert np.load(os.path.join(d, "n_rows.npy")).tolist() == [1.0]


def test_dump_outputs_checksum_and_grouped_order(tmp_path):
    bench = _load("bench", BENCH)
    d = str(tmp_path / "cs")
    cs = 0x995DC9BBDF1939FA
    bench.dump_outputs(d, "cfg4", cs, cs, 7)
    resp = np.load(os.path.join(d, "response_bytes.npy"))
    assert int.from_bytes(bytes(resp.astype(np.uint8)), "big") == cs
    assert not os.path.exists(os.path.join(d, "count.npy"))

    # grouped rows (cfg5 shape: 3 int datums per row) dump identically
    # whatever order the groups came back in
    def row(a, b, g):
        return b"".join(bytes([3]) + (v ^ (1 << 63)).to_bytes(8, "big")
                        for v in (a, b, g))
    rows = [row(5, 50, 2), row(1, 10, 0), row(9, 90, 1)]
    d1, d2 = str(tmp_path / "g1"), str(tmp_path / "g2")
    bench.dump_outputs(d1, "cfg5", 3, b"".join(rows), 3)
    bench.dump_outputs(d2, "cfg5", 3, b"".join(reversed(rows)), 3)
    a = np.load(os.path.join(d1, "response_bytes.npy"))
    b = np.load(os.path.join(d2, "response_bytes.npy"))
    assert a.size == 81 and np.array_equal(a, b)


def test_dump_outputs_large_response_is_a_fixed_sample(tmp_path, monkeypatch):
    bench = _load("bench", BENCH)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    data = np.random.default_rng(7).integers(
        0, 256, size=5000, dtype=np.uint8).tobytes()
    outs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        bench.dump_outputs(d, "cfg2", 1, data, 1)
        outs.append(np.load(os.path.join(d, "response_bytes.npy")))
    assert outs[0].size == 1000 and np.array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_count(tmp_path):
    import tikv_amd
    from tikv_amd import _ffi as F
    bench = _load("bench", BENCH)
    orc = _load("orc_ffi", os.path.join(ROOT, "oracle", "orc_ffi.py"))
    n_rows = 200_003          # not a multiple of any tile size
    gen = tikv_amd.GenRegion(config_index=1, n_rows=n_rows, table_id=1,
                             first_handle=0, n_cols=0)
    try:
        req = bench.build_request(tikv_amd, F, "cfg2")
        o_data, o_n = orc.dag_run(req, gen.keys, gen.key_offs, gen.vals,
                                  gen.val_offs, gen.n_kv)
    finally:
        gen.close()

    d = str(tmp_path / "dump")
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup",
         "1", "--rows", str(n_rows), "--dump-outputs", d],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["metric"] == bench.METRIC["cfg2"]
    assert res["unit"] == "rows/s" and res["dtype"] == "int64"
    assert res["higher_is_better"] is True
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(
        n_rows / (res["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing beyond the headline figure on a plain run
    assert "secondary" not in res and res["cpu_baseline"] is None
    assert "parity gate" not in r.stderr

    resp = np.load(os.path.join(d, "response_bytes.npy"))
    assert bytes(resp.astype(np.uint8)) == o_data
    assert int(np.load(os.path.join(d, "count.npy"))[0]) == \
        bench.parse_count(o_data)
    assert np.load(os.path.join(d, "n_rows.npy")).tolist() == [float(o_n)]
