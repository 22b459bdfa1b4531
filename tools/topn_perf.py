"""TopN wall time (whole copr_dag_run call), single key vs several keys
(DESIGN.md §9f).

Cases, all with n = 100 and output([0, 4, 7]) / all columns:
  a  single key col 4 over GenRegion(config_index=1)       (today's path)
  b  two keys col 4, col 7 over the same region: primary ties are rare, so
     the candidate cut leaves c ~ 100 rows for the second key
  c  two keys over a region built here: column 1 = handle mod 64, column 2 =
     a hash of the handle -- the low-cardinality primary, c ~ m/64 per value

One warm-up call, then `--reps` timed calls; reports each and the median.
dag_run ends in a device-to-host copy, so the host clock brackets finished
work. Needs a GPU; prints its lines and, with --log FILE, appends them there.

  python tools/topn_perf.py --cases a,b --rows 20000000 --tag this
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tikv_amd


def timed(engine, req, rgn, reps):
    engine.dag_run(req, [rgn])                       # warm-up
    ts = []
    nrows = 0
    for _ in range(reps):
        t0 = time.perf_counter()
        data, nrows, _ = engine.dag_run(req, [rgn])
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, nrows


def low_card_region(engine, n_rows):
    """rows {1: handle % 64, 2: hash(handle)} as fixed-width INT datums"""
    import numpy as np
    h = np.arange(n_rows, dtype=np.uint64)
    sign = np.uint64(1 << 63)
    v1 = h % np.uint64(64)
    v2 = (h * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(20)
    vals = np.empty((n_rows, 22), dtype=np.uint8)
    vals[:, 0] = 8; vals[:, 1] = 2; vals[:, 2] = 3       # col id 1, INT flag
    vals[:, 3:11] = (v1 ^ sign).astype(">u8").view(np.uint8).reshape(n_rows, 8)
    vals[:, 11] = 8; vals[:, 12] = 4; vals[:, 13] = 3    # col id 2, INT flag
    vals[:, 14:22] = (v2 ^ sign).astype(">u8").view(np.uint8).reshape(n_rows, 8)
    keys = np.empty((n_rows, 19), dtype=np.uint8)
    keys[:, 0] = ord("t")
    keys[:, 1:9] = np.frombuffer((5).to_bytes(8, "big"), dtype=np.uint8)
    keys[:, 9] = ord("_"); keys[:, 10] = ord("r")
    keys[:, 11:19] = (h ^ sign).astype(">u8").view(np.uint8).reshape(n_rows, 8)
    ko = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(19)
    vo = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(22)
    p8, p64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    return engine.region_raw(keys.ctypes.data_as(p8), ko.ctypes.data_as(p64),
                             vals.ctypes.data_as(p8), vo.ctypes.data_as(p64),
                             n_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    cases = args.cases.split(",")
    E = lambda off: tikv_amd.Expr().col(off)
    eng = tikv_amd.Engine()
    stats = getattr(eng, "topn_stats", lambda: (0, 0, 0))
    out = []

    def report(case, ts, nrows):
        runs, kept, cands = stats()
        line = ("%s case=%s rows=%d out_rows=%d ms=[%s] median=%.1fms "
                "kept=%d candidates=%d" %
                (args.tag, case, args.rows, nrows,
                 ", ".join("%.1f" % t for t in ts), statistics.median(ts),
                 kept if case != "a" else 0, cands if case != "a" else 0))
        print(line, flush=True)
        out.append(line)

    if "a" in cases or "b" in cases:
        g = tikv_amd.GenRegion(config_index=1, n_rows=args.rows, table_id=5)
        rgn = eng.region(g)
        cols = [tikv_amd.Col(i) for i in range(1, 17)]
        if "a" in cases:
            req = (tikv_amd.DagSelect(cols).topn(E(4), 100)
                   .output([0, 4, 7]).build())
            report("a", *timed(eng, req, rgn, args.reps))
        if "b" in cases:
            req = (tikv_amd.DagSelect(cols)
                   .topn([(E(4), False), (E(7), False)], 100)
                   .output([0, 4, 7]).build())
            report("b", *timed(eng, req, rgn, args.reps))
        rgn.close()
        g.close()
    if "c" in cases:
        rgn = low_card_region(eng, args.rows)
        cols = [tikv_amd.Col(1), tikv_amd.Col(2)]
        req = (tikv_amd.DagSelect(cols)
               .topn([(E(0), False), (E(1), False)], 100).build())
        report("c", *timed(eng, req, rgn, args.reps))
        rgn.close()
    eng.close()
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
