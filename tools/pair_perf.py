"""count(*) under two conditions on the cfg2 region, whose 16
int columns all come out as split planes:
  (a) BETWEEN on one column, lo <= c4 < hi: plane_fc_and folds it, and the
      indexed split plane answers from its buckets (k_plane_fcb), beside
      COPR_NO_BUCKETS=1 (k_plane_fcs) and COPR_NO_NARROW=1 (k_plane_fc);
  (b) c4 < x AND c5 >= y over two split columns: k_plane_fc2, beside
      COPR_NO_PAIR=1 (k_plane_agg) and COPR_SPLIT_ALL_LO=1 (every open row
      through the low halves), then three grid caps.
One process; three alternated rounds of the default path and its switches,
each figure the median of `steps` calls: kernel = time_processed_ns, step =
the host clock around the call. The generator has no column narrower than
four bytes beside a wide one, so a 2-byte-and-split shape is not here.

PAIR_PERF_TREE=<checkout> imports tikv_amd from another built tree (the parent
commit, whose switches are then no-ops): run the two trees in alternating
processes for the parent-versus-this figures. Dev tool (GPU box), not part of
the product or bench contract.

usage: pair_perf.py [rows] [steps]
"""
import os
import statistics
import sys
import time

ROOT = os.environ.get("PAIR_PERF_TREE") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def counters(eng):
    pair = getattr(eng, "pair_launches", lambda: 0)()
    return (eng.narrow_stats()[0], eng.split_launches(),
            eng.bucket_stats()[0], pair)


def shape(eng, name, req, rgn, steps, legs, grids=()):
    """legs = (label, switches) pairs, the default path first; every leg of a
    round must give the default's bytes"""
    for rnd in range(3):
        want = None
        for label, sw in legs:
            env(**sw)
            c0 = counters(eng)
            d, k, h = run(eng, req, rgn, steps)
            moved = tuple(b - a for a, b in zip(c0, counters(eng)))
            env(**{key: None for key in sw})
            want = d if want is None else want
            assert d == want, (name, label)
            print("%s round %d %-12s kernel %.4f ms step %.4f ms | narrow/"
                  "split/bucket/pair launches %s | count %s"
                  % (name, rnd, label, k, h, moved, d.hex()), flush=True)
    for g in grids:
        env(COPR_NARROW_GRID=str(g))
        ks = ["%.4f" % run(eng, req, rgn, steps)[1] for _ in range(3)]
        env(COPR_NARROW_GRID=None)
        print("%s grid cap %d: kernel ms %s" % (name, g, " ".join(ks)),
              flush=True)


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    cols = [tikv_amd.Col(i) for i in range(1, 17)]

    def req(*conds):
        return (tikv_amd.DagSelect(cols).where(*conds)
                .simple_agg([tikv_amd.count_star()]).build())

    cmp = tikv_amd.cmp_col_const
    eng = tikv_amd.Engine(0)
    gen = tikv_amd.GenRegion(config_index=1, n_rows=rows, table_id=1)
    print("tree %s: cfg2 region, %d rows" % (ROOT, gen.n_kv), flush=True)
    rgn = eng.region(gen)
    try:
        shape(eng, "between", req(cmp(3, F.SIG_GE_INT, -800_000_000),
                                  cmp(3, F.SIG_LT_INT, -700_000_000)),
              rgn, steps, (("default", {}),
                           ("no_buckets", {"COPR_NO_BUCKETS": "1"}),
                           ("no_narrow", {"COPR_NO_NARROW": "1"})))
        shape(eng, "two_split", req(cmp(3, F.SIG_LT_INT, -800_000_000),
                                    cmp(4, F.SIG_GE_INT, 0)),
              rgn, steps, (("default", {}),
                           ("no_pair", {"COPR_NO_PAIR": "1"}),
                           ("all_lo", {"COPR_SPLIT_ALL_LO": "1"})),
              grids=(512, 768, 1024, 2048))
    finally:
        rgn.close()
        gen.close()
        eng.close()


if __name__ == "__main__":
    main()
