#!/usr/bin/env python3
"""bench.py — TPC-H Q1 on the MI355X fused executor (BASELINE.json metric).

One step = one full Q1 pass (scan+filter+project+hash-agg) over a synthetic
SF10-class lineitem shard resident in HBM (59,986,052 rows per GPU by
default; data generated on-device once, outside the timed region).

N>1 (launched by torch.distributed.run, one rank per GPU over RCCL): weak
scaling — each rank owns a row-range shard of an N x SF10 table (the region-
shard analog, store/copr/coprocessor.go:525); per step each rank runs the
fused kernel in PARTIAL mode and the tiny canonical partial states (~6 groups
x 8 aggs) are all_gather'ed and merged with MergePartialResult semantics
(aggfuncs.go:250-255) — payload is KBs, latency-bound.

Prints ONE JSON line from rank 0 (driver contract).

A plain run sets up, warms up, times the steps and prints the line. The
legs around the headline figure (CPU-oracle baselines, the embedded Q3 SF100
leg) run only with --full. --dump-outputs DIR writes what the last timed
step returned as DIR/<name>.npy (float64) so two builds can be compared
output for output.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

SF10_ROWS = 59_986_052
SF100_ROWS = 599_860_520  # the metric's config (BASELINE.json: Q1 & Q3 SF100)
# algorithmic bytes per row, generated reference layout:
# shipdate 8 + 4 decimals x 40 + 2 char(1) cols x (8 offsets + 1 data);
# synthetic tables carry no null bitmaps (no NULLs) — stated, not 187.
BYTES_PER_ROW = 8 + 4 * 40 + 2 * 1  # dense char(1): offsets proven identity at bind, not read
HBM_PEAK_GBS = 8000.0  # spec peak (MI355X_MICROARCH.md; measured ceiling ~6290)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(msg, file=sys.stderr, flush=True)


Q1_OUT_NAMES = ["returnflag", "linestatus", "sum_qty", "sum_base_price",
                "sum_disc_price", "sum_charge", "avg_qty", "avg_price",
                "avg_disc", "count_order"]
Q3_OUT_NAMES = ["orderkey", "orderdate", "shippriority", "revenue"]


def dump_outputs(dirpath, prefix, names, types, rows):
    """Write decoded result rows column by column as
    dirpath/<prefix>_<name>.npy, float64. Numeric columns (ints, packed
    times, decimals) become a vector, NULL = NaN; string columns become a
    rows x max-bytes matrix of byte codes, padded with -1, NULL row = NaN."""
    import numpy as np
    from tests.gxlib import GX_TYPE_STRING
    assert len(names) == len(types)
    os.makedirs(dirpath, exist_ok=True)
    for c, (name, typ) in enumerate(zip(names, types)):
        vals = [r[c] for r in rows]
        if typ == GX_TYPE_STRING:
            enc = [None if v is None else v.encode() for v in vals]
            width = max([len(b) for b in enc if b is not None] + [1])
            arr = np.full((len(enc), width), -1.0, dtype=np.float64)
            for i, b in enumerate(enc):
                if b is None:
                    arr[i, :] = np.nan
                else:
                    arr[i, :len(b)] = list(b)
        else:
            arr = np.array([np.nan if v is None else float(v) for v in vals],
                           dtype=np.float64)
        np.save(os.path.join(dirpath, f"{prefix}_{name}.npy"), arr)


def run_cpu_baseline(rows=8_000_000):
    """Oracle (CPU restatement) Q1 over pre-generated host-resident chunks —
    the reported baseline, not the target. Two legs: single
    thread, and all host cores via the PARTIAL-per-shard + FINAL-merge split
    (the CPU analog of the multi-GPU merge)."""
    import os
    from tests.gxlib import load_oracle
    lib = load_oracle()
    lib.gx_oracle_bench_q1.argtypes = [
        ctypes.c_int64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]
    lib.gx_oracle_bench_q1_mt.argtypes = [
        ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32,
        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_int64)]
    g = ctypes.c_double()
    e = ctypes.c_double()
    n = ctypes.c_int64()
    rc = lib.gx_oracle_bench_q1(rows, 42, ctypes.byref(g), ctypes.byref(e),
                                ctypes.byref(n))
    if rc != 0:
        return None
    st_rows_s = rows / (e.value / 1000.0)
    cores = os.cpu_count() or 1
    mt_rows = rows * 8 if cores >= 64 else rows  # keep the sample >~1s
    rc = lib.gx_oracle_bench_q1_mt(mt_rows, 42, cores, ctypes.byref(g),
                                   ctypes.byref(e), ctypes.byref(n))
    if rc != 0:
        return None
    return {
        "value": mt_rows / (e.value / 1000.0),
        "unit": "rows/s",
        "cores": cores,
        "kind": "port",
        "single_thread_value": st_rows_s,
        "sample": f"Q1 over {mt_rows} pre-generated host-resident rows, "
                  f"executor only; all-cores = {cores} threads partial+final "
                  f"merge ({e.value/1000:.2f}s); single-thread over {rows} "
                  f"rows = {st_rows_s:.3g} rows/s",
    }


def measured_traffic(metric, rows_this_run):
    """Per-launch HBM bytes from the committed rocprofv3 PMC profile
    (profiles/r01_traffic.json), scaled to this run's row count; None when
    no measurement exists for the metric."""
    import json as _json
    pdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for name in ("r02_traffic.json", "r01_traffic.json"):
        try:
            with open(os.path.join(pdir, name)) as f:
                t = _json.load(f)[metric]
            return t["bytes_per_launch"] * rows_this_run / t["rows_per_launch"]
        except Exception:
            continue
    return None


def run_cpu_baseline_q3(n_li=2_000_000):
    """Oracle Q3 over a bounded sample (~5-10 s of CPU), single thread."""
    import time as _t
    import tests.test_oracle_q3 as q3
    from tests.gxlib import load_oracle
    lib = load_oracle()
    old = (q3.N_LI, q3.N_ORD, q3.N_CUST)
    try:
        q3.N_LI, q3.N_ORD, q3.N_CUST = n_li, n_li // 4, n_li // 40
        t0 = _t.perf_counter()
        q3.run_q3(lib)
        dt = _t.perf_counter() - t0
    finally:
        q3.N_LI, q3.N_ORD, q3.N_CUST = old
    total = n_li + n_li // 4 + n_li // 40
    return {
        "value": total / dt,
        "unit": "rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"Q3 over {n_li} lineitem (+orders/customer) rows incl. "
                  f"generation, single thread ({dt:.1f}s)",
    }


def q3_result(args):
    """TPC-H Q3 (BASELINE config 3): 3-table join + grouped sum + TopN on one
    GPU. One step = the full pipeline (customer/orders build + lineitem probe
    + top-N); tables resident in HBM after the first step."""
    import ctypes as C
    from tests.gxlib import (GX_TPCH_CUSTOMER, GX_TPCH_LINEITEM,
                             GX_TPCH_ORDERS, load_product)
    from tidb_amd import plan as P
    lib = load_product()
    n_li = 6_000_000 * args.sf
    n_ord = n_li // 4
    n_cust = n_ord // 10
    b, (cust, orders, li), topn, out_types, out_fracs = P.q3_plan(lib)
    ex = b.build(topn, device=int(os.environ.get("LOCAL_RANK", "0")))
    ex.bind_tpch(cust, GX_TPCH_CUSTOMER, n_cust)
    ex.bind_tpch(orders, GX_TPCH_ORDERS, n_ord)
    ex.bind_tpch(li, GX_TPCH_LINEITEM, n_li)
    lib.gx_last_kernel_ms.restype = C.c_double
    lib.gx_last_kernel_ms.argtypes = [C.c_void_p]

    def step():
        ex.open()
        rows = ex.pull_all(out_types, out_fracs, data_caps=[None] * 4)
        ex.close()
        return rows, lib.gx_last_kernel_ms(ex.ex)

    t0 = time.perf_counter()
    for i in range(args.warmup):
        rows, _ = step()
        if i == 0:
            log(f"[bench] q3 first step (incl. generation of {n_li} lineitem"
                f" rows): {time.perf_counter()-t0:.1f}s, {len(rows)} rows")
    t0 = time.perf_counter()
    kms = []
    for _ in range(args.steps):
        rows, k = step()
        kms.append(k)
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "q3", Q3_OUT_NAMES, out_types, rows)
    total_rows = n_li + n_ord + n_cust
    value = total_rows * args.steps / elapsed
    # probe-kernel roofline: algorithmic bytes per lineitem row on the Q3
    # probe: shipdate 8 + orderkey 8 + extendedprice 40 + discount 40 = 96 B
    # sequential + random slot traffic (reported separately via counters)
    probe_bpr = 96
    avg_kms = sum(kms) / len(kms)
    achieved = n_li * probe_bpr / (avg_kms / 1000.0) / 1e9 if avg_kms else 0
    out = {
        "metric": "tpch_q3_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int128",
        "data": "synthetic",
        "config": {
            "workload": f"tpch_q3_sf{args.sf}_synthetic",
            "lineitem_rows": n_li,
            "orders_rows": n_ord,
            "customer_rows": n_cust,
            "parallelism": "single-gpu",
            "probe_bytes_per_row": probe_bpr,
        },
        "probe_kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": run_cpu_baseline_q3() if not args.no_cpu_baseline
        else None,
        "result_rows": len(rows),
    }
    ex.free()
    b.free()
    return out


def bench_q3(args):
    print(json.dumps(q3_result(args)), flush=True)


def run_cpu_baseline_sort(n=1_000_000):
    """Oracle full sort over a bounded sample, single thread."""
    import time as _t
    from tests.test_full_sort import run_sort, KEYS_2
    from tests.gxlib import load_oracle
    lib = load_oracle()
    t0 = _t.perf_counter()
    run_sort(lib, KEYS_2, [0, 0], n_rows=n)
    dt = _t.perf_counter() - t0
    return {
        "value": n / dt,
        "unit": "rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"full sort of {n} lineitem rows incl. generation and "
                  f"result pull, single thread ({dt:.1f}s)",
    }


def bench_sort(args):
    """Full ORDER BY over lineitem (sortexec/sort.go analog):
    device radix sort by (l_shipdate, l_orderkey) + full-table gather. One
    step = compose keys + 2 stable radix passes + gather of all 8 columns
    (kernel time via gx_last_kernel_ms; table stays resident)."""
    import ctypes as C
    from tests.gxlib import (GX_TPCH_LINEITEM, GX_TYPE_I64, GX_TYPE_TIME,
                             load_product)
    from tidb_amd import plan as P
    lib = load_product()
    n = args.rows
    lib.gx_last_kernel_ms.restype = C.c_double
    lib.gx_last_kernel_ms.argtypes = [C.c_void_p]

    def step():
        bb = P.Builder(lib)
        src = bb.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
        keys = [bb.colref(P.L_SHIPDATE, GX_TYPE_TIME),
                bb.colref(P.L_ORDERKEY, GX_TYPE_I64)]
        root = bb.sort(src, keys, [0, 0])
        ex = bb.build(root)
        ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
        ex.open()
        out_types = P.LINEITEM_TYPES
        chunk = ex.pull_one(out_types, P.LINEITEM_FRACS,
                            data_caps=[None] * 5 + [2048, 2048] + [None])
        k = lib.gx_last_kernel_ms(ex.ex)
        ex.close()
        ex.free()
        bb.free()
        return chunk, k

    for i in range(args.warmup):
        step()
    t0 = time.perf_counter()
    kms = []
    for _ in range(args.steps):
        _, k = step()
        kms.append(k)
    elapsed = time.perf_counter() - t0
    avg_kms = sum(kms) / len(kms)
    value = n / (avg_kms / 1000.0) if avg_kms else 0
    # algorithmic bytes/row: keys read twice (2 passes x 8B gathered reads) +
    # pair sort traffic (~4 radix passes x 12B rw) + full-table gather
    # read+write (170 x 2); dominated by the gather
    bpr = 2 * 8 + 4 * 24 + 2 * 170
    achieved = n * bpr / (avg_kms / 1000.0) / 1e9 if avg_kms else 0
    out = {
        "metric": "lineitem_sort_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": f"lineitem_sort_{n}_by_shipdate_orderkey",
            "rows": n,
            "parallelism": "single-gpu",
            "bytes_per_row": bpr,
        },
        "sort_kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": run_cpu_baseline_sort() if not args.no_cpu_baseline
        else None,
    }
    print(json.dumps(out), flush=True)


def bench_wide(args):
    """Wide projection (BASELINE config 5's shape at round-1 VM capacity):
    15 chained decimal expressions over 4 columns feeding 7 sums + count,
    through the hipRTC-specialized kernel. One step = one pass over the
    resident lineitem shard."""
    import ctypes as C
    from tests.gxlib import GX_TPCH_LINEITEM, load_product
    from tests.test_wide_projection import wide_plan
    lib = load_product()
    n = args.rows
    lib.gx_last_kernel_ms.restype = C.c_double
    lib.gx_last_kernel_ms.argtypes = [C.c_void_p]
    b, src, agg, out_types, out_fracs = wide_plan(lib)
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)

    def step():
        ex.open()
        caps = [2048 if t == 4 else None for t in out_types]
        rows = ex.pull_all(out_types, out_fracs, data_caps=caps)
        k = lib.gx_last_kernel_ms(ex.ex)
        ex.close()
        return rows, k

    for _ in range(args.warmup):
        step()
    t0 = time.perf_counter()
    kms = []
    rows = []
    for _ in range(args.steps):
        rows, k = step()
        kms.append(k)
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "wide",
                     [f"col{c}" for c in range(len(out_types))], out_types,
                     rows)
    avg_kms = sum(kms) / len(kms)
    value = n / (avg_kms / 1000.0) if avg_kms else 0
    bpr = 170  # same resident lineitem shard as Q1
    achieved = n * bpr / (avg_kms / 1000.0) / 1e9 if avg_kms else 0
    out = {
        "metric": "wide_projection_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int128",
        "data": "synthetic",
        "config": {
            "workload": f"wide_projection_15expr_8agg_{n}_rows",
            "rows": n,
            "parallelism": "single-gpu",
            "bytes_per_row": bpr,
        },
        "kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": None,
    }
    ex.free()
    b.free()
    print(json.dumps(out), flush=True)


def run_cpu_baseline_join(n_li=4_000_000):
    """Oracle standalone join over a bounded sample, single thread."""
    import time as _t
    from tests.gxlib import (GX_TPCH_LINEITEM, GX_TPCH_ORDERS, GX_TYPE_I64,
                             load_oracle)
    from tidb_amd import plan as P
    lib = load_oracle()
    n_ord = n_li // 4
    t0 = _t.perf_counter()
    b = P.Builder(lib)
    orders = b.source(P.ORDERS_TYPES)
    li = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    j = b.hashjoin(orders, li, [b.colref(P.O_ORDERKEY, GX_TYPE_I64)],
                   [b.colref(P.L_ORDERKEY, GX_TYPE_I64)])
    ex = b.build(j)
    ex.bind_tpch(orders, GX_TPCH_ORDERS, n_ord)
    ex.bind_tpch(li, GX_TPCH_LINEITEM, n_li)
    ex.open()
    # drive Next to EOF without Python-decoding every row
    import ctypes as C
    from tidb_amd.chunkpy import PyChunk
    out_types = P.ORDERS_TYPES + P.LINEITEM_TYPES
    out_fracs = [0] * 4 + P.LINEITEM_FRACS
    chunk = PyChunk(out_types, 1024, out_fracs)
    total = 0
    while True:
        g = chunk.as_gx()
        n = C.c_int32(0)
        rc = lib.gx_next(ex.ex, C.byref(g), C.byref(n))
        assert rc == 0, ex.error()
        if n.value == 0:
            break
        total += n.value
    ex.close()
    ex.free()
    b.free()
    dt = _t.perf_counter() - t0
    return {
        "value": (n_li + n_ord) / dt,
        "unit": "rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"orders({n_ord}) JOIN lineitem({n_li}) on orderkey incl. "
                  f"generation, {total} joined rows, single thread ({dt:.1f}s)",
    }


def bench_join(args):
    """Standalone inner hash join (hash_join_v2.go):
    orders (build) ⋈ lineitem (probe) on orderkey, joined rows MATERIALIZED
    on device (build cols ++ probe cols gathered through the match index).
    One step = chain build + count + fill + gather of all 12 output columns
    over freshly generated tables (kernel time via HIP events around the
    join phases; generation excluded)."""
    import ctypes as C
    from tests.gxlib import (GX_TPCH_LINEITEM, GX_TPCH_ORDERS, GX_TYPE_I64,
                             load_product)
    from tidb_amd import plan as P
    lib = load_product()
    # cap at SF50: the SF100 12-column materialization (~270 GB incl. the
    # joined output) sits at the 288 GB edge and would take the graceful
    # out-of-core path — this bench measures the IN-MEMORY join
    n_li = min(args.rows, 299_930_260)
    n_ord = n_li // 4
    lib.gx_last_kernel_ms.restype = C.c_double
    lib.gx_last_kernel_ms.argtypes = [C.c_void_p]
    lib.gx_last_sel_count.restype = C.c_int64
    lib.gx_last_sel_count.argtypes = [C.c_void_p]

    out_types = P.ORDERS_TYPES + P.LINEITEM_TYPES
    out_fracs = [0] * 4 + P.LINEITEM_FRACS

    def step():
        # fresh executor per step: device buffers (output table ~13 GB at
        # SF10) are freed with it
        b = P.Builder(lib)
        orders = b.source(P.ORDERS_TYPES)
        li = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
        j = b.hashjoin(orders, li, [b.colref(P.O_ORDERKEY, GX_TYPE_I64)],
                       [b.colref(P.L_ORDERKEY, GX_TYPE_I64)])
        ex = b.build(j)
        ex.bind_tpch(orders, GX_TPCH_ORDERS, n_ord)
        ex.bind_tpch(li, GX_TPCH_LINEITEM, n_li)
        ex.open()
        ex.pull_one(out_types, out_fracs,
                    data_caps=[None] * 9 + [2048, 2048, None])
        k = lib.gx_last_kernel_ms(ex.ex)
        matches = lib.gx_last_sel_count(ex.ex)
        ex.close()
        ex.free()
        b.free()
        return k, matches

    for _ in range(args.warmup):
        step()
    t0 = time.perf_counter()
    kms = []
    matches = 0
    for _ in range(args.steps):
        k, matches = step()
        kms.append(k)
    elapsed = time.perf_counter() - t0
    avg_kms = sum(kms) / len(kms)
    value = (n_li + n_ord) / (avg_kms / 1000.0) if avg_kms else 0
    # algorithmic bytes per matched row (≈ per probe row here: every lineitem
    # matches its order): probe side read 178 (8B key+time + 4x40 dec + 2
    # dense char) + build side random read 32 (4x8B) + output write 210 +
    # match-pair index write+read 16; plus per probe row: head probe 4 +
    # next walk 4
    bpr_out = 178 + 32 + 210 + 16
    achieved = (matches * bpr_out + n_li * 8) / (avg_kms / 1000.0) / 1e9 \
        if avg_kms else 0
    out = {
        "metric": "hash_join_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": f"orders_{n_ord}_join_lineitem_{n_li}_materialized",
            "lineitem_rows": n_li,
            "orders_rows": n_ord,
            "joined_rows": matches,
            "parallelism": "single-gpu",
            "bytes_per_joined_row": bpr_out,
        },
        "join_kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": run_cpu_baseline_join() if not args.no_cpu_baseline
        else None,
    }
    print(json.dumps(out), flush=True)


def run_cpu_baseline_strings(n=2_000_000):
    """Oracle string-builtin projection over a bounded customer sample."""
    import time as _t
    from tests.gxlib import GX_TPCH_CUSTOMER, load_oracle
    lib = load_oracle()
    t0 = _t.perf_counter()
    b, src, root = _strings_plan(lib)
    ex = b.build(root)
    ex.bind_tpch(src, GX_TPCH_CUSTOMER, n)
    ex.open()
    import ctypes as C
    from tests.gxlib import GX_TYPE_STRING
    from tidb_amd.chunkpy import PyChunk
    types = [4, 4, 0, 0]
    chunk = PyChunk(types, 1024, [0] * 4, [32768, 32768, None, None])
    total = 0
    while True:
        g = chunk.as_gx()
        nn = C.c_int32(0)
        rc = lib.gx_next(ex.ex, C.byref(g), C.byref(nn))
        assert rc == 0, ex.error()
        if nn.value == 0:
            break
        total += nn.value
    ex.close()
    ex.free()
    b.free()
    dt = _t.perf_counter() - t0
    return {
        "value": n / dt,
        "unit": "rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"SUBSTR/UPPER/LENGTH projection over {n} customer rows "
                  f"incl. generation and pull, single thread ({dt:.1f}s)",
    }


def _strings_plan(lib):
    """Varchar-builtin projection (config 5's varchar half): SUBSTR(seg,1,4),
    UPPER(SUBSTR(seg,-5,5)), LENGTH(seg), custkey over customer."""
    from tests.gxlib import (GX_F_LENGTH, GX_F_SUBSTR, GX_F_UPPER,
                             GX_TYPE_I64, GX_TYPE_STRING)
    from tidb_amd import plan as P
    b = P.Builder(lib)
    src = b.source(P.CUSTOMER_TYPES)
    seg = b.colref(P.C_MKTSEGMENT, GX_TYPE_STRING)
    exprs = [
        b.call(GX_F_SUBSTR, GX_TYPE_STRING, 0, seg, b.const_i64(1),
               b.const_i64(4)),
        b.call(GX_F_UPPER, GX_TYPE_STRING, 0,
               b.call(GX_F_SUBSTR, GX_TYPE_STRING, 0, seg, b.const_i64(-5),
                      b.const_i64(5))),
        b.call(GX_F_LENGTH, GX_TYPE_I64, 0, seg),
        b.colref(P.C_CUSTKEY, GX_TYPE_I64),
    ]
    root = b.projection(src, exprs)
    return b, src, root


def bench_strings(args):
    """Varchar builtins at scale (BASELINE config 5's varchar half,
    SURVEY §8f row 2): a 4-expression string projection (2 windowed string
    outputs + LENGTH + passthrough key) over `--rows` synthetic customer
    rows resident in HBM. One step = the full device projection (window
    kernels + offset scans + byte emits); emission to host excluded."""
    import ctypes as C
    from tests.gxlib import GX_TPCH_CUSTOMER, load_product
    lib = load_product()
    n = min(args.rows, 150_000_000)
    lib.gx_last_kernel_ms.restype = C.c_double
    lib.gx_last_kernel_ms.argtypes = [C.c_void_p]
    b, src, root = _strings_plan(lib)
    ex = b.build(root)
    ex.bind_tpch(src, GX_TPCH_CUSTOMER, n)

    def step():
        ex.open()
        ex.pull_one([4, 4, 0, 0], [0] * 4,
                    data_caps=[32768, 32768, None, None])
        k = lib.gx_last_kernel_ms(ex.ex)
        ex.close()
        return k

    for _ in range(args.warmup):
        step()
    t0 = time.perf_counter()
    kms = []
    for _ in range(args.steps):
        kms.append(step())
    elapsed = time.perf_counter() - t0
    avg_kms = sum(kms) / len(kms)
    value = n / (avg_kms / 1000.0) if avg_kms else 0
    # algorithmic bytes/row: offsets 8 + segment bytes ~12.9 read by window
    # (data read once per string output at emit: 2 x ~5) + key 8 + temps
    # (start/len/notNull 17 x 2 outputs, written+read) + out writes (~9 + 8)
    bpr = 8 + 13 + 8 + 2 * 5 + 2 * 2 * 17 + 9 + 8 + 8
    achieved = n * bpr / (avg_kms / 1000.0) / 1e9 if avg_kms else 0
    out = {
        "metric": "string_builtin_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {
            "workload": f"customer_{n}_substr_upper_length_projection",
            "rows": n,
            "parallelism": "single-gpu",
            "bytes_per_row": bpr,
        },
        "kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": run_cpu_baseline_strings()
        if not args.no_cpu_baseline else None,
    }
    ex.free()
    b.free()
    print(json.dumps(out), flush=True)


def run_cpu_baseline_groupby(n=2_000_000):
    """Oracle 3-col group-by over a bounded lineitem sample."""
    import time as _t
    from tests.gxlib import load_oracle
    lib = load_oracle()
    t0 = _t.perf_counter()
    _run_groupby_plan(lib, n)
    dt = _t.perf_counter() - t0
    return {
        "value": n / dt,
        "unit": "rows/s",
        "cores": 1,
        "kind": "port",
        "sample": f"3-col group-by over {n} lineitem rows incl. generation "
                  f"and pull, single thread ({dt:.1f}s)",
    }


def _run_groupby_plan(lib, n, device=0):
    from tests.gxlib import (GX_AGG_COUNT, GX_AGG_SUM, GX_TPCH_LINEITEM,
                             GX_TYPE_DECIMAL, GX_TYPE_I64, GX_TYPE_STRING)
    from tidb_amd import plan as P
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    groups = [b.colref(P.L_RETFLAG, GX_TYPE_STRING),
              b.colref(P.L_LINESTATUS, GX_TYPE_STRING),
              b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2)]
    agg = b.hashagg(src, groups,
                    [(GX_AGG_SUM, b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                      2), (GX_AGG_COUNT, -1, 0)])
    ex = b.build(agg, device=device)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
    ex.open()
    out_types = [GX_TYPE_STRING, GX_TYPE_STRING, GX_TYPE_DECIMAL,
                 GX_TYPE_DECIMAL, GX_TYPE_I64]
    rows = 0
    import ctypes as C
    from tidb_amd.chunkpy import PyChunk
    chunk = PyChunk(out_types, 1024, [0, 0, 2, 2, 0], [4096, 4096, None,
                                                       None, None])
    while True:
        g = chunk.as_gx()
        nn = C.c_int32(0)
        rc = lib.gx_next(ex.ex, C.byref(g), C.byref(nn))
        assert rc == 0, ex.error()
        if nn.value == 0:
            break
        rows += nn.value
    k = None
    try:
        lib.gx_last_kernel_ms.restype = C.c_double
        lib.gx_last_kernel_ms.argtypes = [C.c_void_p]
        k = lib.gx_last_kernel_ms(ex.ex)
    except Exception:
        pass
    ex.close()
    ex.free()
    b.free()
    return rows, k


def bench_groupby(args):
    """Serialized-key group-by (SURVEY §8a rows 9-10 generality): group
    lineitem by (returnflag, linestatus, quantity) — the decimal key forces
    the wide-key path (hash + record-verified, interpreted kernel), 600
    groups. One step = one full pass incl. group decode. (1M+ NDV parity
    lives in tests/test_wide_groupkeys.py; extreme NDV ~ rows degenerates
    to distinct-materialization and is not a throughput workload.)"""
    from tests.gxlib import load_product
    lib = load_product()
    n = min(args.rows, 59_986_052)  # group decode is host-side O(NDV)
    for _ in range(args.warmup):
        _run_groupby_plan(lib, n)
    t0 = time.perf_counter()
    kms = []
    ng = 0
    for _ in range(args.steps):
        ng, k = _run_groupby_plan(lib, n)
        kms.append(k or 0)
    elapsed = time.perf_counter() - t0
    avg_kms = sum(kms) / len(kms)
    value = n / (avg_kms / 1000.0) if avg_kms else 0
    # algorithmic bytes/row: qty 16 (DEC16 fetch; key and sum share the
    # load) + 2 chars 2 + offsets pairs 2 x 16 for the string keys'
    # trimmed-window reads; record traffic is cached (600 groups)
    bpr = 16 + 2 + 32
    achieved = n * bpr / (avg_kms / 1000.0) / 1e9 if avg_kms else 0
    out = {
        "metric": "wide_groupby_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int128",
        "data": "synthetic",
        "config": {
            "workload": f"lineitem_{n}_groupby_rf_ls_quantity_wide_keys",
            "rows": n,
            "groups": ng,
            "parallelism": "single-gpu",
            "bytes_per_row": bpr,
        },
        "kernel_ms_avg": avg_kms,
        "roofline": {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": None,
        },
        "cpu_baseline": run_cpu_baseline_groupby()
        if not args.no_cpu_baseline else None,
    }
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=SF100_ROWS,
                    help="rows per GPU (default SF100 — the metric's config)")
    ap.add_argument("--query",
                    choices=["q1", "q3", "sort", "wide", "join", "strings",
                             "groupby"],
                    default="q1")
    ap.add_argument("--sf", type=int, default=100,
                    help="scale factor for --query q3 (lineitem = 6M x SF)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs around the headline figure: the "
                         "CPU-oracle baseline and, for q1 on one GPU, the "
                         "embedded Q3 SF100 leg")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU-oracle baseline")
    ap.add_argument("--no-q3", action="store_true",
                    help="with --full: skip the embedded Q3 SF100 leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as "
                         "DIR/<name>.npy (float64); --query q1, q3 and wide")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.query not in ("q1", "q3", "wide"):
        ap.error("--dump-outputs: --query %s hands no rows back to the "
                 "caller" % args.query)
    if not args.full:
        args.no_cpu_baseline = True
        args.no_q3 = True

    if args.query == "q3":
        return bench_q3(args)
    if args.query == "sort":
        return bench_sort(args)
    if args.query == "wide":
        return bench_wide(args)
    if args.query == "join":
        return bench_join(args)
    if args.query == "strings":
        return bench_strings(args)
    if args.query == "groupby":
        return bench_groupby(args)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = world if world > 1 else args.gpus

    dist = None
    if world > 1:
        import torch
        import torch.distributed as tdist
        backend = os.environ.get("GX_BENCH_BACKEND", "nccl")  # nccl = RCCL
        if torch.cuda.is_available():
            # identity on a full node; lets a 2-rank smoke run on 1 GPU (gloo)
            local_rank = local_rank % torch.cuda.device_count()
            torch.cuda.set_device(local_rank)
        tdist.init_process_group(backend)
        dist = tdist

    from tests.gxlib import (GX_AGG_MODE_COMPLETE, GX_AGG_MODE_PARTIAL,
                             GX_TPCH_LINEITEM, load_product)
    from tidb_amd import plan as P
    from tests.test_dist_merge import merge_partials

    lib = load_product()
    mode = GX_AGG_MODE_PARTIAL if world > 1 else GX_AGG_MODE_COMPLETE
    b, src, agg, out_types, out_fracs = P.q1_plan(lib, mode)
    ex = b.build(agg, device=local_rank)
    total_rows = args.rows * n_gpus
    ex.bind_tpch(src, GX_TPCH_LINEITEM, args.rows, seed=42,
                 row_offset=rank * args.rows, total_rows=total_rows)
    caps = [2048 if t == 4 else None for t in out_types]

    lib.gx_last_kernel_ms.restype = ctypes.c_double
    lib.gx_last_kernel_ms.argtypes = [ctypes.c_void_p]
    lib.gx_last_sel_count.restype = ctypes.c_int64
    lib.gx_last_sel_count.argtypes = [ctypes.c_void_p]

    from tidb_amd.chunkpy import PyChunk
    bench_chunk = PyChunk(out_types, 1024, out_fracs, caps)

    def step():
        ex.open()
        rows = ex.pull_all(out_types, out_fracs, data_caps=caps,
                           reuse_chunk=bench_chunk)
        ex.close()
        if world > 1:
            # partial states travel as wire-codec bytes in DEVICE tensors
            # (RCCL over xGMI; gloo host tensors in CPU smoke runs) —
            # tidb_amd/dist.py, the ShuffleExec/partial-worker analog
            from tidb_amd import dist as gxdist
            all_rows = gxdist.gather_partial_rows(dist, lib, out_types,
                                                  out_fracs, rows)
            result = merge_partials(lib, all_rows)
        else:
            result = {(r[0], r[1]): tuple(r[2:]) for r in rows}
        return result, lib.gx_last_kernel_ms(ex.ex)

    def sync():
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        except Exception:
            pass
        if world > 1:
            dist.barrier()

    t_gen0 = time.perf_counter()
    for i in range(args.warmup):
        result, _ = step()
        if i == 0:
            log(f"[bench] first step (incl. on-device generation of "
                f"{args.rows} rows): {time.perf_counter()-t_gen0:.1f}s, "
                f"{len(result)} groups")
    sync()
    t0 = time.perf_counter()
    kernel_ms = []
    result = None
    for _ in range(args.steps):
        result, kms = step()
        kernel_ms.append(kms)
    sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if world > 1:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank != 0:
        return

    if args.dump_outputs:
        # group order out of the hash table is not part of the result
        q1_rows = sorted((k + v for k, v in result.items()),
                         key=lambda r: tuple(x or "" for x in r[:2]))
        # merged (N>1) and COMPLETE results share the final schema
        dump_outputs(args.dump_outputs, "q1", Q1_OUT_NAMES,
                     [4, 4] + [2] * 7 + [0], q1_rows)

    ms_per_step = elapsed / args.steps * 1000.0
    value = (args.rows * n_gpus) * args.steps / elapsed
    gbs_scanned = value * BYTES_PER_ROW / 1e9

    avg_kms = sum(kernel_ms) / len(kernel_ms) if kernel_ms else 0
    roofline = None
    if avg_kms > 0:
        achieved_gbs = args.rows * BYTES_PER_ROW / (avg_kms / 1000.0) / 1e9
        roofline = {
            "bound": "hbm",
            "achieved": achieved_gbs,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved_gbs / HBM_PEAK_GBS,
            # per-launch HBM bytes from the committed rocprofv3 PMC profile
            "traffic": measured_traffic("tpch_q1_rows_per_sec", args.rows),
        }

    cpu_baseline = None
    if n_gpus == 1 and not args.no_cpu_baseline:
        log("[bench] timing CPU baseline (oracle, single thread)...")
        cpu_baseline = run_cpu_baseline()

    # second headline config (BASELINE config 3): Q3 SF100 in the same
    # driver-attested line. The Q1 tables (~102 GB at SF100) are freed first
    # so both fit comfortably in 288 GB HBM.
    q3 = None
    if n_gpus == 1 and not args.no_q3:
        ex.free()
        b.free()
        ex = b = None
        log("[bench] running embedded Q3 SF100 leg...")
        import copy
        q3_args = copy.copy(args)
        q3_args.sf = 100
        q3_args.steps = min(args.steps, 10)
        q3_args.warmup = min(args.warmup, 2)
        try:
            q3 = q3_result(q3_args)
        except Exception as e:  # the Q1 headline line must still print
            log(f"[bench] q3 leg failed: {e}")
            q3 = {"error": str(e)}

    out = {
        "metric": "tpch_q1_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int128",
        "data": "synthetic",
        "config": {
            "workload": f"tpch_q1_sf{round(args.rows / (SF10_ROWS / 10))}"
                        "_synthetic_lineitem",
            "rows_per_gpu": args.rows,
            "parallelism": f"shard-dp{n_gpus}+partial-merge",
            "bytes_per_row": BYTES_PER_ROW,
        },
        "gb_per_sec_scanned": gbs_scanned,
        "kernel_ms_avg": avg_kms,
        "roofline": roofline,
        "cpu_baseline": cpu_baseline,
        "groups": len(result) if result else 0,
        "q3_sf100": q3,
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
