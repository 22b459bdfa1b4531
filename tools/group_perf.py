"""Hash-aggregation wall time (whole copr_dag_run call), one group-by column
vs several.

Cases:
  a   cfg3's own request (count(*), sum(decimal), avg(key) BY key) over the
      cfg3 region as bench.py --workload cfg3 builds it: the single-key path,
      comparable between a parent build and this one
  a2  one key over the region built here: columns 1 and 2 are int keys of 64
      and 8 distinct values, column 3 an int value; count(*), sum(col 3),
      avg(col 1) BY col 1. The cfg3 region has one int column only, so the
      multi-key cases need a region of their own, and a2 is their single-key
      yardstick on it.
  b   the same aggregates BY col 1, col 2 on that region: plane key source,
      k_plane_hash route
  c   case b with COPR_NO_PLANES=1: row-bytes key source, sorted route

One warm-up call, then `--reps` timed calls; reports each and the median.
dag_run ends in a device-to-host copy, so the host clock brackets finished
work. Needs a GPU; prints its lines and, with --log FILE, appends them there.

  python tools/group_perf.py --cases a,a2,b,c --rows 20000000 --tag this
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tikv_amd
from tikv_amd import _ffi as F


def timed(engine, req, rgn, reps):
    engine.dag_run(req, [rgn])                       # warm-up
    ts = []
    nrows = 0
    for _ in range(reps):
        t0 = time.perf_counter()
        data, nrows, _ = engine.dag_run(req, [rgn])
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, nrows


def two_key_region(engine, n_rows):
    """rows {1: h % 64, 2: (h // 64) % 8, 3: hash(h)} as fixed-width INT
    datums, 33 value bytes per row"""
    import numpy as np
    h = np.arange(n_rows, dtype=np.uint64)
    sign = np.uint64(1 << 63)
    v = [h % np.uint64(64), (h // np.uint64(64)) % np.uint64(8),
         (h * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)]
    vals = np.empty((n_rows, 33), dtype=np.uint8)
    for c in range(3):
        o = 11 * c
        vals[:, o] = 8; vals[:, o + 1] = 2 * (c + 1); vals[:, o + 2] = 3
        vals[:, o + 3:o + 11] = ((v[c] ^ sign).astype(">u8").view(np.uint8)
                                 .reshape(n_rows, 8))
    keys = np.empty((n_rows, 19), dtype=np.uint8)
    keys[:, 0] = ord("t")
    keys[:, 1:9] = np.frombuffer((5).to_bytes(8, "big"), dtype=np.uint8)
    keys[:, 9] = ord("_"); keys[:, 10] = ord("r")
    keys[:, 11:19] = (h ^ sign).astype(">u8").view(np.uint8).reshape(n_rows, 8)
    ko = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(19)
    vo = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(33)
    p8, p64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    return engine.region_raw(keys.ctypes.data_as(p8), ko.ctypes.data_as(p64),
                             vals.ctypes.data_as(p8), vo.ctypes.data_as(p64),
                             n_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,a2,b,c")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    cases = args.cases.split(",")
    E = lambda off: tikv_amd.Expr().col(off)
    eng = tikv_amd.Engine()
    stats = getattr(eng, "group_stats", lambda: (0, 0, 0, 0))
    out = []

    def report(case, ts, nrows):
        line = ("%s case=%s rows=%d out_rows=%d ms=[%s] median=%.1fms "
                "group_stats=%s hash_plane_launches=%d" %
                (args.tag, case, args.rows, nrows,
                 ", ".join("%.1f" % t for t in ts), statistics.median(ts),
                 stats(), eng.hash_plane_launches()))
        print(line, flush=True)
        out.append(line)

    if "a" in cases:
        g = tikv_amd.GenRegion(config_index=2, n_rows=args.rows, table_id=1,
                               n_cols=64)
        rgn = eng.region(g)
        cols = [tikv_amd.Col(1), tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=2),
                tikv_amd.Col(3, tp=F.TP_VARCHAR)]
        req = tikv_amd.DagSelect(cols).hash_agg(
            [tikv_amd.count_star(), tikv_amd.sum_col(1, decimal=2),
             tikv_amd.avg_col(0)], E(0)).build()
        report("a", *timed(eng, req, rgn, args.reps))
        rgn.close()
        g.close()
    if {"a2", "b", "c"} & set(cases):
        rgn = two_key_region(eng, args.rows)
        cols = [tikv_amd.Col(1), tikv_amd.Col(2), tikv_amd.Col(3)]
        aggs = lambda: [tikv_amd.count_star(), tikv_amd.sum_col(2),
                        tikv_amd.avg_col(0)]
        if "a2" in cases:
            req = tikv_amd.DagSelect(cols).hash_agg(aggs(), E(0)).build()
            report("a2", *timed(eng, req, rgn, args.reps))
        if "b" in cases or "c" in cases:
            req = tikv_amd.DagSelect(cols).hash_agg(aggs(), [E(0), E(1)]).build()
            if "b" in cases:
                report("b", *timed(eng, req, rgn, args.reps))
            if "c" in cases:
                os.environ["COPR_NO_PLANES"] = "1"
                try:
                    report("c", *timed(eng, req, rgn, args.reps))
                finally:
                    del os.environ["COPR_NO_PLANES"]
        rgn.close()
    eng.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
