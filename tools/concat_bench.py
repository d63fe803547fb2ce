#!/usr/bin/env python3
"""Composed-string projection vs the single-column window path, on device.

Over the synthetic customer table of `bench.py --query strings` (same default
row count), timed with gx_last_kernel_ms, three plans in ONE process:

  A  UPPER(c_mktsegment)                      window path (strWindow/strEmit)
  B  CONCAT(UPPER(c_mktsegment))              composed path, the same bytes
  C  CONCAT(c_mktsegment, '-', CAST_STR(c_custkey))

After a warm-up the plans run alternately (A, B, C, A, B, C, ...) for
--reps rounds; one JSON line per plan reports the median, minimum and
maximum kernel ms and the algorithmic bytes per row worked out from the
shapes. Before timing, A and B must agree on the first 1024 rows.

  python tools/concat_bench.py [--rows N] [--reps 10] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests.gxlib import (GX_F_UPPER, GX_TPCH_CUSTOMER, GX_TYPE_I64,  # noqa: E402
                         GX_TYPE_STRING, load_product)
from tidb_amd import plan as P  # noqa: E402
from tidb_amd.chunkpy import PyChunk  # noqa: E402

STRINGS_BENCH_ROWS = 150_000_000  # bench.py --query strings at its default
SEGMENT_BYTES = (10 + 8 + 9 + 9 + 9) / 5  # AUTOMOBILE BUILDING FURNITURE
#                                           MACHINERY HOUSEHOLD, equally likely


def avg_key_digits(n):
    """Mean decimal digits of c_custkey = 1..n."""
    total, lo, d = 0, 1, 1
    while lo <= n:
        hi = min(n, lo * 10 - 1)
        total += (hi - lo + 1) * d
        lo, d = lo * 10, d + 1
    return total / n


def bytes_per_row(plan, n):
    """Algorithmic HBM bytes per row, from the shapes alone."""
    seg = SEGMENT_BYTES
    scan = 8 + 8               # lens read, offsets written
    nulls = 1 + 1 / 8          # notNull read, bitmap written
    if plan == "A":
        # window: offsets read, (start, len, notNull) written; emit: temps
        # and out offsets read, source bytes read, output bytes written
        return 8 + 17 + scan + 17 + 8 + seg + seg + nulls
    # length pass: source offsets read, 9 B lens + notNull written; emit:
    # source offsets and out offsets read, source bytes read, output written
    out = seg
    src = 8 + 8 + seg
    if plan == "C":
        out = seg + 1 + avg_key_digits(n)
        src += 8 + 8           # c_custkey read by both passes
    return src + 9 + scan + 8 + out + nulls


def build(lib, plan):
    b = P.Builder(lib)
    src = b.source(P.CUSTOMER_TYPES)
    seg = b.colref(P.C_MKTSEGMENT, GX_TYPE_STRING)
    up = b.call(GX_F_UPPER, GX_TYPE_STRING, 0, seg)
    if plan == "A":
        e = up
    elif plan == "B":
        e = b.call(P.GX_F_CONCAT, GX_TYPE_STRING, 0, up)
    else:
        cast = b.call(P.GX_F_CAST_STR, GX_TYPE_STRING, 0,
                      b.colref(P.C_CUSTKEY, GX_TYPE_I64))
        e = b.call(P.GX_F_CONCAT, GX_TYPE_STRING, 0, seg, b.const_str("-"),
                   cast)
    ex = b.build(b.projection(src, [e]))
    assert ex.error() == "", ex.error()
    return b, src, ex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=STRINGS_BENCH_ROWS)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    lib = load_product()
    lib.gx_last_kernel_ms.restype = ctypes.c_double
    lib.gx_last_kernel_ms.argtypes = [ctypes.c_void_p]
    n = args.rows
    plans = {}
    for name in "ABC":
        b, src, ex = build(lib, name)
        ex.bind_tpch(src, GX_TPCH_CUSTOMER, n)
        plans[name] = (b, ex)

    def first_rows(ex):
        ex.open()
        chunk = PyChunk([GX_TYPE_STRING], 1024, [0], [1 << 16])
        g = chunk.as_gx()
        got = ctypes.c_int32(0)
        rc = lib.gx_next(ex.ex, ctypes.byref(g), ctypes.byref(got))
        assert rc == 0, ex.error()
        rows = chunk.rows(got.value)
        ex.close()
        return rows

    def step(ex):
        ex.open()
        ex.pull_one([GX_TYPE_STRING], [0], data_caps=[1 << 16])
        ms = lib.gx_last_kernel_ms(ex.ex)
        ex.close()
        return ms

    a_rows, b_rows = first_rows(plans["A"][1]), first_rows(plans["B"][1])
    assert len(a_rows) == min(n, 1024) and a_rows == b_rows, \
        "plans A and B disagree on the first 1024 rows"
    c_rows = first_rows(plans["C"][1])
    assert c_rows[0][0].endswith("-1") and c_rows[-1][0].endswith(
        "-" + str(len(c_rows))), c_rows[:2]

    for _ in range(args.warmup):
        for name in "ABC":
            step(plans[name][1])
    ms = {name: [] for name in "ABC"}
    for _ in range(args.reps):
        for name in "ABC":
            ms[name].append(step(plans[name][1]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name in "ABC":
        bpr = bytes_per_row(name, n)
        line = {
            "plan": name,
            "rows": n,
            "reps": args.reps,
            "kernel_ms_median": med[name],
            "kernel_ms_min": min(ms[name]),
            "kernel_ms_max": max(ms[name]),
            "bytes_per_row": round(bpr, 2),
            "gb_per_s": round(n * bpr / (med[name] / 1000.0) / 1e9, 1)
            if med[name] else None,
        }
        if name == "B":
            line["b_over_a"] = round(med["B"] / med["A"], 3) if med["A"] else None
        print(json.dumps(line), flush=True)
    for b, ex in plans.values():
        ex.free()
        b.free()


if __name__ == "__main__":
    main()
