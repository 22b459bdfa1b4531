"""The filter+count step's own clock beside the host's: runs
the benchmark's cfg2 request over one resident region, 5 warm-up calls and 20
timed ones, and prints for each timed call the kernel's time_processed_ns and
the host-clock time of the call. Run it under a kernel tracer and the last 20
k_plane_fcs dispatches (k_plane_fcb on a plane with a bucket index,
DESIGN.md §9q) of the trace are these 20 calls: tracer's duration
minus time_processed_ns is the dispatch ramp the in-kernel figure leaves out,
and the check on "block 0 first". Dev tool (GPU box), not part of the product
or bench contract.

usage: fc_step_probe.py [rows] [out.csv]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tikv_amd
from tikv_amd import _ffi as F

import bench


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else bench.N_ROWS_DEFAULT
    out = sys.argv[2] if len(sys.argv) > 2 else None
    gen = tikv_amd.GenRegion(config_index=1, n_rows=rows, table_id=1)
    eng = tikv_amd.Engine(0)
    rgn = eng.region(gen)
    req = bench.build_request(tikv_amd, F, "cfg2", 3)
    lines = ["call,time_processed_ns,host_ns"]
    try:
        for _ in range(5):
            eng.dag_run(req, [rgn])
        w0 = eng.fc_wait_stats()
        for i in range(20):
            t0 = time.perf_counter_ns()
            _, _, kns = eng.dag_run(req, [rgn])
            lines.append("%d,%d,%d" % (i, kns, time.perf_counter_ns() - t0))
        w1 = eng.fc_wait_stats()
    finally:
        rgn.close()
        eng.close()
        gen.close()
    print("\n".join(lines))
    print("polled %d, fallbacks %d" % (w1[0] - w0[0], w1[1] - w0[1]))
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
