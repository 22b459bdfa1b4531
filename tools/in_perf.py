"""IN-list filters over the column planes against the scan path and their
comparison kernels: count(*) WHERE col IN (8 items) on the
cfg2 region's filter column (wide planes: k_plane_in, beside k_plane_fc under
COPR_NO_NARROW=1 for a >= filter) and on a cfg3 generator region whose group
column lies in 0..59999 and again in 0..199 (2- and 1-byte planes:
k_plane_inb, beside k_plane_fcn). Then the split plane:
k_plane_ins against COPR_NO_IN_SPLIT=1, which is k_plane_in, beside
k_plane_fcs, on the cfg2 column with 8 and with 1024 items and on a generator
column of range 70000 with keys in both of its buckets. One process; three
alternated pairs of the plane path and its switch, each figure the median of
`steps` calls: kernel = time_processed_ns, step = the host clock around the
call. IN_PERF_ONLY=split runs the split sections alone. Run it under a
kernel tracer for the tracer's durations. Dev tool (GPU box), not part of the
product or bench contract.

usage: in_perf.py [rows_wide] [rows_narrow] [steps]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tikv_amd
from tikv_amd import _ffi as F


def env(**kw):
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def run(eng, req, rgn, steps, warm=5):
    for _ in range(warm):
        data = eng.dag_run(req, [rgn])[0]
    kns, host = [], []
    for _ in range(steps):
        t0 = time.perf_counter_ns()
        d, _, k = eng.dag_run(req, [rgn])
        host.append(time.perf_counter_ns() - t0)
        kns.append(k)
        assert d == data
    return data, statistics.median(kns) / 1e6, statistics.median(host) / 1e6


def count_req(cols, sel):
    return (tikv_amd.DagSelect(cols).where(sel)
            .simple_agg([tikv_amd.count_star()]).build())


def section(eng, name, gen, cols, off, items, ge_const, bytes_per_row, steps,
            stat, ge_env, switch="COPR_NO_IN_PLANES", grids=()):
    """stat = index into in_stats(), or None for in_split_launches();
    switch = what turns the measured path off for the other half of a pair;
    grids = COPR_IN_GRID caps to time afterwards, three runs each"""
    count = (lambda: eng.in_stats()[stat]) if stat is not None \
        else eng.in_split_launches
    rgn = eng.region(gen)
    n = gen.n_kv
    try:
        req_in = count_req(cols, tikv_amd.in_col_consts(off, items))
        req_ge = count_req(cols, tikv_amd.cmp_col_const(off, F.SIG_GE_INT,
                                                        ge_const))
        for pair in range(3):
            env(**{switch: None})
            s0 = count()
            d1, k1, h1 = run(eng, req_in, rgn, steps)
            assert count() > s0, "plane kernel did not run"
            env(**{switch: "1"})
            s0 = count()
            d2, k2, h2 = run(eng, req_in, rgn, steps)
            assert count() == s0, "%s=1 was not read" % switch
            env(**{switch: None})
            assert d1 == d2
            print("%s pair %d: planes kernel %.4f ms step %.4f ms | %s "
                  "kernel %.4f ms step %.4f ms, ratio %.3f / %.3f | %.1f GB/s "
                  "| count %s"
                  % (name, pair, k1, h1, switch, k2, h2, k2 / k1, h2 / h1,
                     n * bytes_per_row / k1 / 1e6, d1.hex()), flush=True)
            env(**ge_env)
            _, k3, h3 = run(eng, req_ge, rgn, steps)
            env(**{k: None for k in ge_env})
            print("%s pair %d: >= kernel %.4f ms step %.4f ms, ratio IN/>= "
                  "%.3f" % (name, pair, k3, h3, k1 / k3), flush=True)
        for g in grids:
            env(COPR_IN_GRID=str(g))
            ks = ["%.4f" % run(eng, req_in, rgn, steps)[1] for _ in range(3)]
            env(COPR_IN_GRID=None)
            print("%s grid cap %d: kernel ms %s" % (name, g, " ".join(ks)),
                  flush=True)
    finally:
        rgn.close()


def main():
    rows_w = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    rows_n = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    only = os.environ.get("IN_PERF_ONLY")
    eng = tikv_amd.Engine(0)
    try:
        gen = tikv_amd.GenRegion(config_index=1, n_rows=rows_w, table_id=1)
        cols2 = [tikv_amd.Col(i) for i in range(1, 17)]
        items = [-800_000_000 + 7 * i for i in range(8)]
        if only != "split":
            print("wide: cfg2 region, %d rows" % gen.n_kv, flush=True)
            env(COPR_NO_IN_SPLIT="1")
            section(eng, "wide", gen, cols2, 3, items, 800_000_000, 9, steps,
                    0, {"COPR_NO_NARROW": "1"})
            env(COPR_NO_IN_SPLIT=None)
        # split plane: bytes per row = the 2 B of high halves every row reads
        print("split: cfg2 region, %d rows" % gen.n_kv, flush=True)
        section(eng, "split8", gen, cols2, 3, items, 800_000_000, 2, steps,
                None, {}, "COPR_NO_IN_SPLIT", grids=(512, 768, 1024, 2048))
        many = [-1_000_000_000 + 1_953_125 * i + 11 for i in range(1024)]
        section(eng, "split1024", gen, cols2, 3, many, 800_000_000, 2, steps,
                None, {}, "COPR_NO_IN_SPLIT", grids=(512, 768, 1024, 2048))
        gen.close()
        gen = tikv_amd.GenRegion(config_index=2, n_rows=rows_n, table_id=1,
                                 n_cols=70000)
        print("split dense: cfg3 region, group column in 0..69999, %d rows"
              % gen.n_kv, flush=True)
        cols = [tikv_amd.Col(1),
                tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=2),
                tikv_amd.Col(3, tp=F.TP_VARCHAR)]
        section(eng, "split_dense", gen, cols, 0,
                [5, 77, 1000, 31999, 65535, 65536, 69999, -4], 54000, 4, steps,
                None, {}, "COPR_NO_IN_SPLIT", grids=(512, 768, 1024, 2048))
        gen.close()
        if only == "split":
            return
        gen = tikv_amd.GenRegion(config_index=2, n_rows=rows_n, table_id=1,
                                 n_cols=60000)
        print("bitmap: cfg3 region, group column in 0..59999, %d rows"
              % gen.n_kv, flush=True)
        cols = [tikv_amd.Col(1),
                tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=2),
                tikv_amd.Col(3, tp=F.TP_VARCHAR)]
        section(eng, "bitmap", gen, cols, 0, [5, 77, 1000, 31999, 32000, 59999,
                                              60000, -4], 54000, 2, steps, 1, {})
        gen.close()
        gen = tikv_amd.GenRegion(config_index=2, n_rows=rows_n, table_id=1,
                                 n_cols=200)
        print("bitmap1: cfg3 region, group column in 0..199, %d rows"
              % gen.n_kv, flush=True)
        section(eng, "bitmap1", gen, cols, 0, [5, 31, 32, 77, 150, 199, 200, -4],
                180, 1, steps, 1, {})
        gen.close()
    finally:
        eng.close()


if __name__ == "__main__":
    main()
