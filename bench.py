#!/usr/bin/env python3
"""bench.py — coprocessor rows/sec on the BASELINE workloads (contract bench).

N=1 primary workload = BASELINE.json configs[1]: 100 M-row x 16-i64-column
synthetic region, TableScan + Selection(col3 < k @10% selectivity) + count(*),
on one MI355X. A "step" is one full pass of the fused scan/filter/agg hot
path over the HBM-resident region. A plain run does only what that headline
figure needs: generate + ingest the region, warm up, time --steps passes,
print the result line.

--full (single GPU) adds everything else the benchmark measures or checks:
the secondary BASELINE workloads (cfg3 hash-agg, cfg4 CRC64 checksum), whose
full result objects are attached under "secondary" in the same JSON line,
each with its own metric text, roofline and cpu_baseline; and the parity
gate: after warmup the full region is run through the CPU oracle and
compared against the GPU response — bit-exact for cfg2/cfg4,
order-insensitive grouped rows for cfg3 (group output order is not part of
parity). The timed gate run doubles as the cpu_baseline
sample.

--dump-outputs DIR writes what the last timed step of the primary workload
returned to its caller as DIR/<name>.npy (see dump_outputs). Inputs are a
pure function of the arguments (copr_gen.cpp RNG contract), so two builds
can be compared output for output.

Multi-GPU: one process per GPU (torchrun), each rank owns its own Region
shard (weak scaling — Regions are disjoint key ranges, exactly TiDB's
per-Region fan-out, endpoint.rs:238-248); the only exchange is the final
count merge (one u64 all_reduce).

Output: ONE JSON line from rank 0 (see the repo task contract).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_ROWS_DEFAULT = 100_000_000
FILTER_K = -800_000_000          # 10% selectivity over uniform ±1e9
HBM_PEAK_GBS = 8000.0            # 8 TB/s spec (MI355X_MICROARCH.md)

METRIC = {
    "cfg2": "coprocessor rows/sec (scan+filter+count)",
    "cfg3": "coprocessor rows/sec (scan+hash-agg count/sum(dec)/avg BY col0)",
    "cfg4": "checksum KV pairs/sec (CRC64-XOR)",
    "cfg5": "coprocessor rows/sec (index-scan+filter+hash-agg)",
}
UNIT = {"cfg2": "rows/s", "cfg3": "rows/s", "cfg4": "KV/s", "cfg5": "rows/s"}
DTYPE = {"cfg2": "int64", "cfg3": "int64", "cfg4": "u64", "cfg5": "int64"}
DESC = {
    "cfg2": "cfg2: 100M-row i64x16 TableScan + Selection(col3<k, 10%) + count(*)",
    "cfg3": "cfg3: mixed i64/Decimal/VarBytes TableScan + HashAgg(count,sum,avg BY col0, K=64)",
    "cfg4": "cfg4: CRC64-XOR checksum over KV pairs",
    "cfg5": "cfg5: secondary IndexScan + Selection + HashAgg",
}


def log(msg):
    sys.stderr.write("[bench] %s\n" % msg)
    sys.stderr.flush()


def load_oracle():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "orc_ffi", os.path.join(ROOT, "oracle", "orc_ffi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_request(tikv_amd, F, workload, filter_offset=3):
    if workload == "cfg2":
        cols = [tikv_amd.Col(i) for i in range(1, 17)]
        sel = tikv_amd.cmp_col_const(filter_offset, F.SIG_LT_INT, FILTER_K)
        return (tikv_amd.DagSelect(cols).where(sel)
                .simple_agg([tikv_amd.count_star()]).build())
    if workload == "cfg3":
        cols = [tikv_amd.Col(1),
                tikv_amd.Col(2, tp=F.TP_NEWDECIMAL, decimal=2),
                tikv_amd.Col(3, tp=F.TP_VARCHAR)]
        return tikv_amd.DagSelect(cols).hash_agg(
            [tikv_amd.count_star(), tikv_amd.sum_col(1, decimal=2),
             tikv_amd.avg_col(0)], tikv_amd.Expr().col(0)).build()
    if workload == "cfg5":
        cols = [tikv_amd.Col(1), tikv_amd.Col(2),
                tikv_amd.Col(-1, pk_handle=True)]
        sel = tikv_amd.cmp_col_const(1, F.SIG_GE_INT, 0)
        return (tikv_amd.DagSelect(cols, index=True).where(sel)
                .hash_agg([tikv_amd.count_star(), tikv_amd.sum_col(1)],
                          tikv_amd.Expr().col(0)).build())
    return None     # cfg4: checksum request, no DAG


def parse_count(data):
    assert len(data) == 9 and data[0] == 3
    return int.from_bytes(data[1:9], "big") ^ (1 << 63)


def split_datum_rows(data, datums_per_row):
    """split a TypeDefault datum response into row byte strings
    (flag lengths per datum.rs:1117-1155; enough for int/dec/bytes)"""
    D2B = [0, 1, 1, 2, 2, 3, 3, 4, 4, 4]
    rows, i, cur, ncol = [], 0, [], 0
    while i < len(data):
        start = i
        flag = data[i]
        i += 1
        if flag == 0:
            pass
        elif flag in (3, 4, 5, 7):
            i += 8
        elif flag in (8, 9):
            while data[i] & 0x80:
                i += 1
            i += 1
        elif flag == 6:
            prec, frac = data[i], data[i + 1]
            ic = prec - frac
            i += 2 + (ic // 9) * 4 + D2B[ic % 9] + (frac // 9) * 4 + D2B[frac % 9]
        elif flag == 2:
            ln, shift = 0, 0
            while True:
                b = data[i]
                i += 1
                ln |= (b & 0x7F) << shift
                shift += 7
                if b < 0x80:
                    break
            i += ln >> 1
        else:
            raise AssertionError("datum flag %d" % flag)
        cur.append(data[start:i])
        ncol += 1
        if ncol == datums_per_row:
            rows.append(b"".join(cur))
            cur, ncol = [], 0
    assert not cur
    return rows


def read_traffic(workload, n_rows):
    """Per-launch HBM bytes measured offline with rocprofv3 --pmc (FETCH_SIZE
    x2 gfx950 correction + WRITE_SIZE, per MI355X_MICROARCH.md §HBM), stored
    by tools/roofline.py into profiles/pmc_traffic.json. None if absent."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(p) as f:
            d = json.load(f)
        t = d.get("%s_hbm_bytes_per_launch" % workload)
        if t is None and workload == "cfg2":
            t = d.get("cfg2_scan_hbm_bytes_per_launch")
        if t is None:
            return None
        ref_rows = d.get("%s_rows" % workload, N_ROWS_DEFAULT)
        return t * (n_rows / ref_rows)
    except Exception:
        return None


DUMP_MAX_BYTES = 8 << 20          # response bytes kept (x4 as float32 = 32 MB)


def dump_outputs(out_dir, workload, headline, data, n_out):
    """Write the last timed step's caller-visible outputs as float .npy:

    response_bytes.npy  f32  the encoded response, one element per byte
                             (cfg4: the u64 checksum, 8 big-endian bytes).
                             Grouped responses (cfg3/cfg5) are written with
                             their rows sorted bytewise: group output order
                             is not part of the contract.
    n_rows.npy          f64  rows in the response (cfg4: KV pairs summed)
    count.npy           f64  cfg2 only: the decoded count(*) (< 2^53, exact)

    A response longer than DUMP_MAX_BYTES is sampled at fixed seeded
    positions, so the files stay comparable between runs and under 64 MB."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    if workload == "cfg4":
        data = int(headline).to_bytes(8, "big")
    elif workload in ("cfg3", "cfg5"):
        data = b"".join(sorted(split_datum_rows(
            data, 5 if workload == "cfg3" else 3)))
    b = np.frombuffer(data, dtype=np.uint8)
    if b.size > DUMP_MAX_BYTES:
        idx = np.random.default_rng(0).choice(
            b.size, size=DUMP_MAX_BYTES, replace=False)
        idx.sort()
        b = b[idx]
    np.save(os.path.join(out_dir, "response_bytes.npy"),
            b.astype(np.float32))
    np.save(os.path.join(out_dir, "n_rows.npy"),
            np.array([n_out], dtype=np.float64))
    if workload == "cfg2":
        np.save(os.path.join(out_dir, "count.npy"),
                np.array([headline], dtype=np.float64))


def bench_one(tikv_amd, F, eng, workload, n_rows, steps, warmup,
              world, rank, dist, have_cuda, parity, filter_offset=3,
              dump_dir=None):
    """Run one workload end-to-end; returns the result dict (rank 0) and the
    merged headline count. Region/generator are freed before returning."""
    log("rank %d/%d: generating %d rows (%s shape)"
        % (rank, world, n_rows, workload))
    t0 = time.perf_counter()
    gen = tikv_amd.GenRegion(
        config_index={"cfg2": 1, "cfg3": 2, "cfg4": 3, "cfg5": 4}[workload],
        n_rows=n_rows, table_id=1, first_handle=rank * n_rows,
        n_cols=64 if workload == "cfg3" else 0)
    log("generated in %.1fs (%.2f GB values)"
        % (time.perf_counter() - t0, gen.val_bytes() / 1e9))
    req = build_request(tikv_amd, F, workload, filter_offset)
    rgn = eng.region(gen)

    # algorithmic bytes per pass: every encoded value byte once + the
    # val_offs the kernel reads (8 B per row boundary) + the cell-directory
    # planes the kernel reads (1 B per row per referenced column, built at
    # ingest; COPR_NO_DIR drops them and the kernel's read together). Keys
    # are only read by the checksum (cfg4) and index scans (cfg5).
    # 
    algo_bytes = gen.val_bytes() + 8 * (gen.n_kv + 1)
    if not os.environ.get("COPR_NO_DIR"):
        if workload == "cfg2":
            algo_bytes += gen.n_kv          # filter column plane
        elif workload == "cfg3":
            algo_bytes += 3 * gen.n_kv      # group + sum + avg column planes
    if workload == "cfg4":
        algo_bytes += gen.key_bytes() + 8 * (gen.n_kv + 1)
    elif workload == "cfg5":
        # index scans parse the KEY stream
        algo_bytes = gen.key_bytes() + 8 * (gen.n_kv + 1)

    def step():
        """one pass; returns (raw_data, n_out, kernel_ns): the response (or
        the u64 checksum), its row count (KV pairs for cfg4), kernel time"""
        if workload == "cfg4":
            cs, kvs, byts = eng.checksum([rgn])
            return cs, kvs, 0
        return eng.dag_run(req, [rgn])

    def headline(data, n_out):
        if workload == "cfg2":
            return parse_count(data)
        return data if workload == "cfg4" else n_out

    cnt = None
    g_data = None
    for _ in range(max(warmup, 1)):   # >=1: the parity gate needs a result
        g_data, g_n, _ = step()
        cnt = headline(g_data, g_n)

    # ---- full-scale parity gate (assert at BASELINE size).
    # The timed oracle pass doubles as the cpu_baseline sample (kind "port",
    # 1 thread). Only rank 0 at N=1 (the contract's cpu_baseline scope).
    cpu = None
    if rank == 0 and world == 1 and parity:
        orc = load_oracle()
        log("parity gate: oracle full pass over %d rows (%s) ..."
            % (gen.n_kv, workload))
        t0 = time.perf_counter()
        if workload == "cfg4":
            o_cs, o_kvs, o_bytes = orc.checksum(
                gen.keys, gen.key_offs, gen.vals, gen.val_offs, gen.n_kv)
            dt = time.perf_counter() - t0
            assert o_cs == g_data, \
                "cfg4 checksum mismatch GPU=%x oracle=%x" % (g_data, o_cs)
        else:
            o_data, o_n = orc.dag_run(req, gen.keys, gen.key_offs,
                                      gen.vals, gen.val_offs, gen.n_kv)
            dt = time.perf_counter() - t0
            if workload == "cfg2":
                assert o_data == g_data and o_n == 1, "cfg2 response mismatch"
            elif workload == "cfg3":
                # 5 datums/row: count, sum_dec, avg_cnt, avg_sum, group
                assert sorted(split_datum_rows(o_data, 5)) == \
                    sorted(split_datum_rows(g_data, 5)), \
                    "cfg3 grouped results mismatch"
            elif workload == "cfg5":
                # 3 datums/row: count, sum, group
                assert sorted(split_datum_rows(o_data, 3)) == \
                    sorted(split_datum_rows(g_data, 3)), \
                    "cfg5 grouped results mismatch"
        log("parity gate ok (%.1fs)" % dt)
        cpu = {"value": gen.n_kv / dt, "unit": UNIT[workload], "cores": 1,
               "kind": "port",
               "sample": "full region (%d rows), the parity-gate oracle pass,"
                         " 1 thread" % gen.n_kv}

    if dist and workload == "cfg2":
        if getattr(eng, "_comm_ranks", 0) == world:
            # the engine's own RCCL merge over xGMI (copr_merge_count) — the
            # data-path collective lives in libcopr.so, not torch
            cnt = eng.merge_count(cnt)
        else:
            import torch
            t = torch.tensor([cnt], dtype=torch.long)
            dist.all_reduce(t)        # oversubscribed dev boxes: gloo
            cnt = int(t.item())

    # timed region (each step already ends with a hipStreamSynchronize inside
    # copr_dag_run; torch sync covers any torch-side stream)
    import torch
    if dist:
        dist.barrier()
    if have_cuda:
        torch.cuda.synchronize()
    kern_ns_total = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        last_data, last_n, kns = step()
        kern_ns_total += kns
    if have_cuda:
        torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed])   # timing plumbing rides the gloo group
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_rows = n_rows * world * steps
    rows_per_sec = total_rows / elapsed
    ms_per_step = elapsed / steps * 1e3
    kern_s = kern_ns_total / 1e9 / steps
    if workload == "cfg4" or kern_s <= 0:
        kern_s = elapsed / steps     # checksum call is synchronous
    achieved_gbs = algo_bytes / kern_s / 1e9

    if dump_dir and rank == 0:
        dump_outputs(dump_dir, workload, headline(last_data, last_n),
                     last_data, last_n)
        log("outputs of the last timed step written to %s" % dump_dir)

    result = None
    if rank == 0:
        result = {
            "metric": METRIC[workload],
            "value": rows_per_sec,
            "unit": UNIT[workload],
            "n_gpus": world,
            "steps": steps,
            "warmup": warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": DTYPE[workload],
            "data": "synthetic",
            "config": {
                "workload": DESC[workload],
                "rows_per_gpu": n_rows,
                "selectivity": 0.1 if workload == "cfg2" else None,
                "parallelism": "region-sharded dp%d" % world,
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved_gbs,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved_gbs / HBM_PEAK_GBS,
                "traffic": read_traffic(workload, n_rows),
            },
            "cpu_baseline": cpu,
        }
    rgn.close()
    gen.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=N_ROWS_DEFAULT,
                    help="rows per GPU (dev override; BASELINE value default)")
    ap.add_argument("--filter-offset", type=int, default=3,
                    help="dev: which column offset the predicate filters")
    ap.add_argument("--full", action="store_true",
                    help="also run the parity gate + cpu_baseline oracle "
                         "pass and the secondary cfg3/cfg4 lines (N=1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs of the primary "
                         "workload as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the parity gate + cpu_baseline "
                         "oracle pass")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary cfg3/cfg4 lines")
    ap.add_argument("--workload", default=None,
                    choices=["cfg2", "cfg3", "cfg4", "cfg5"],
                    help="bench ONLY this workload (default: the cfg2 "
                         "contract line; --full attaches cfg3/cfg4 "
                         "secondary lines at N=1)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    # torch first: initialize HIP device discovery before the engine's own
    # runtime use in this process
    import torch
    have_cuda = torch.cuda.is_available()

    import tikv_amd
    from tikv_amd import _ffi as F

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as tdist
        # gloo is BOOTSTRAP + timing plumbing only (comm-id broadcast,
        # elapsed-max); the data-path collective is the engine's own RCCL
        # merge (copr_comm.cpp), created below
        tdist.init_process_group(backend="gloo")
        dist = tdist

    n_dev = torch.cuda.device_count() if have_cuda else 1
    dev = local_rank % max(n_dev, 1)
    eng = tikv_amd.Engine(dev)
    if have_cuda:
        torch.cuda.set_device(dev)
    if dist and have_cuda and world <= n_dev:
        # one GPU per rank: the engine's RCCL communicator over xGMI
        obj = [tikv_amd.Engine.comm_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        eng.comm_create(obj[0], world, rank)
        eng._comm_ranks = world
        log("rank %d: engine RCCL communicator up (world %d)" % (rank, world))

    primary = args.workload or "cfg2"
    # parity gate (--full): oracle at full bench size is ~25-40 s of host
    # CPU; --no-cpu-baseline drops it from a --full run. cfg5's gate is
    # covered by the GPU test suite instead (index parity tests).
    gate = args.full and not args.no_cpu_baseline
    parity = gate and primary != "cfg5"
    result = bench_one(tikv_amd, F, eng, primary, args.rows, args.steps,
                       args.warmup, world, rank, dist, have_cuda, parity,
                       args.filter_offset, args.dump_outputs)

    # secondary BASELINE lines (hash-agg + checksum) on a single-process
    # --full invocation — VERDICT r01: driver-measurable cfg3/cfg4
    if (args.full and args.workload is None and world == 1
            and not args.no_secondary):
        secondary = []
        for w in ("cfg3", "cfg4"):
            r = bench_one(tikv_amd, F, eng, w, args.rows,
                          max(args.steps // 2, 3), max(args.warmup // 2, 2),
                          world, rank, dist, have_cuda, gate)
            if r is not None:
                secondary.append(r)
        if result is not None:
            result["secondary"] = secondary

    if rank == 0 and result is not None:
        print(json.dumps(result))
    eng.close()
    if dist:
        dist.destroy_process_group()
    return result


if __name__ == "__main__":
    main()
