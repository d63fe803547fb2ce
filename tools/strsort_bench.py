#!/usr/bin/env python3
"""Device ORDER BY over the synthetic customer table: what the string rank
costs on top of the int64-keyed sort of the same rows.

Two plans over customer (c_custkey int64, c_mktsegment varchar), timed with
gx_last_kernel_ms (device events around the whole sort: rank build, LSD
chain, column gathers) in ONE process:

  K  ORDER BY c_custkey                  the existing chain plus the varlen
                                         payload gather
  S  ORDER BY c_mktsegment, c_custkey    plus the rank of c_mktsegment

After a warm-up the plans run alternately (K, S, K, S, ...) for --reps
rounds, each run on a fresh executor (generate, then sort at the first
Next); one JSON line per plan reports the median, minimum and maximum kernel
ms. S also reports the refinement rounds of its rank build (read from
the engine's GX_DEBUG line of one extra, untimed run) and s_minus_k, the cost
of building and using the rank. Before timing, the first 1024 rows of each
plan are checked: K ascends by key, S by (segment, key).

  python tools/strsort_bench.py [--rows N] [--reps 5] [--warmup 1]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests.gxlib import GX_TPCH_CUSTOMER, load_product  # noqa: E402
from tidb_amd import plan as P  # noqa: E402
from tidb_amd.chunkpy import PyChunk  # noqa: E402

DEFAULT_ROWS = 15_000_000
KEYS = {"K": [P.C_CUSTKEY], "S": [P.C_MKTSEGMENT, P.C_CUSTKEY]}


def build(lib, plan, n):
    b = P.Builder(lib)
    src = b.source(P.CUSTOMER_TYPES)
    keys = [b.colref(c, P.CUSTOMER_TYPES[c]) for c in KEYS[plan]]
    ex = b.build(b.sort(src, keys, [0] * len(keys)))
    assert ex.error() == "", ex.error()
    ex.bind_tpch(src, GX_TPCH_CUSTOMER, n)
    return b, ex


def run_once(lib, plan, n, want_rows=False):
    """A fresh executor (a sorted bare source stays sorted across re-open):
    generate, sort at the first Next, return (kernel ms, first rows)."""
    b, ex = build(lib, plan, n)
    ex.open()
    chunk = PyChunk(P.CUSTOMER_TYPES, 1024, None, [None, 1 << 16])
    g = chunk.as_gx()
    got = ctypes.c_int32(0)
    rc = lib.gx_next(ex.ex, ctypes.byref(g), ctypes.byref(got))
    assert rc == 0, ex.error()
    ms = lib.gx_last_kernel_ms(ex.ex)
    rows = chunk.rows(got.value) if want_rows else None
    ex.close()
    ex.free()
    b.free()
    return ms, rows


def rounds_from_debug(lib, n):
    """One untimed run of plan S with GX_DEBUG set and stderr in a file."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["GX_DEBUG"] = "1"
        try:
            run_once(lib, "S", n)
        finally:
            del os.environ["GX_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode("utf8", "replace")
    m = re.search(r"string rank: .* (\d+) refinement rounds", text)
    return int(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=DEFAULT_ROWS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    lib = load_product()
    lib.gx_last_kernel_ms.restype = ctypes.c_double
    lib.gx_last_kernel_ms.argtypes = [ctypes.c_void_p]
    n = args.rows

    _, k_rows = run_once(lib, "K", n, want_rows=True)
    assert len(k_rows) == min(n, 1024) and \
        k_rows == sorted(k_rows, key=lambda r: r[0]), "plan K is not ordered"
    _, s_rows = run_once(lib, "S", n, want_rows=True)
    assert len(s_rows) == min(n, 1024) and \
        s_rows == sorted(s_rows, key=lambda r: (r[1].encode(), r[0])), \
        "plan S is not ordered"
    rounds = rounds_from_debug(lib, n)

    for _ in range(args.warmup):
        for name in KEYS:
            run_once(lib, name, n)
    ms = {name: [] for name in KEYS}
    for _ in range(args.reps):
        for name in KEYS:
            ms[name].append(run_once(lib, name, n)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    for name in KEYS:
        line = {
            "plan": name,
            "order_by": ["c_custkey", "c_mktsegment"][KEYS[name][0]] +
            (", c_custkey" if len(KEYS[name]) > 1 else ""),
            "rows": n,
            "reps": args.reps,
            "kernel_ms_median": round(med[name], 3),
            "kernel_ms_min": round(min(ms[name]), 3),
            "kernel_ms_max": round(max(ms[name]), 3),
        }
        if name == "S":
            line["refinement_rounds"] = rounds
            line["s_minus_k_ms"] = round(med["S"] - med["K"], 3)
            line["s_over_k"] = round(med["S"] / med["K"], 3) if med["K"] else None
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
