"""Lane-replicated LDS accumulators: the generated fused
kernels keep R copies of each group's accumulators in LDS and a lane adds
into copy threadIdx.x & (R-1); the copies are folded before the flush. A
block that meets more keys than the small table holds sends the executor to
the single-copy 64-slot layout (tier 1), and from there the older chain goes
on to global-direct accumulation (tier 2). Results must stay exactly the
oracle's on every tier, and every case asserts on gx_debug_lds_tier so none
can pass on a fallback.
"""
import ctypes

import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_AGG_MAX, GX_AGG_MIN, GX_AGG_SUM,
                         GX_TPCH_LINEITEM, GX_TYPE_DECIMAL, GX_TYPE_I64,
                         load_oracle, load_product)
from tests.test_wide_projection import wide_plan
from tidb_amd import plan as P

pytestmark = pytest.mark.gpu

# wave (64), block (256) and 2-deep-pipeline (512) edges of a 256-thread block
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 513, 5000]


@pytest.fixture(scope="module")
def libs():
    return load_oracle(), load_product()


def lds_tier(lib, ex):
    lib.gx_debug_lds_tier.restype = ctypes.c_int32
    lib.gx_debug_lds_tier.argtypes = [ctypes.c_void_p]
    return lib.gx_debug_lds_tier(ex.ex)


def repl_slots(lib, ex):
    lib.gx_debug_lds_repl_slots.restype = ctypes.c_int32
    lib.gx_debug_lds_repl_slots.argtypes = [ctypes.c_void_p]
    return lib.gx_debug_lds_repl_slots(ex.ex)


def run_plan(lib, plan, bind, opens=1, product=False):
    """`opens` open/pull/close cycles on ONE executor. Returns the sorted rows
    of each cycle and, for the product engine, the tier after each cycle and
    the replicated table's slot count."""
    b, src, agg, out_types, out_fracs = plan(lib)
    ex = b.build(agg)
    bind(ex, src)
    caps = [2048 if t == 4 else None for t in out_types]
    results, tiers, slots = [], [], None
    try:
        for _ in range(opens):
            ex.open()
            rows = ex.pull_all(out_types, out_fracs, data_caps=caps)
            ex.close()
            results.append(sorted(rows, key=repr))
            if product:
                tiers.append(lds_tier(lib, ex))
        if product:
            slots = repl_slots(lib, ex)
    finally:
        ex.free()
        b.free()
    return results, tiers, slots


def _tpch(n):
    return lambda ex, src: ex.bind_tpch(src, GX_TPCH_LINEITEM, n)


_oracle_cache = {}


def _oracle(oracle, name, plan, bind):
    if name not in _oracle_cache:  # one oracle run per input, shared
        _oracle_cache[name] = run_plan(oracle, plan, bind)[0][0]
    return _oracle_cache[name]


# ---- Q1 edge sizes ---------------------------------------------------------

@pytest.mark.parametrize("mode,tier", [("jit", 0), ("no_jit", 1),
                                       ("no_repl", 1)])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_q1_edge_sizes(libs, monkeypatch, n, mode, tier):
    oracle, product = libs
    if mode == "no_jit":
        monkeypatch.setenv("GX_NO_JIT", "1")
    elif mode == "no_repl":
        monkeypatch.setenv("GX_NO_LDS_REPL", "1")
    opens = 2 if n == 5000 else 1
    got, tiers, _ = run_plan(product, P.q1_plan, _tpch(n), opens=opens,
                             product=True)
    want = _oracle(oracle, ("q1", n), P.q1_plan, _tpch(n))
    assert tiers == [tier] * opens
    for g in got:
        assert g == want


# ---- no group key ----------------------------------------------------------

@pytest.mark.parametrize("n", [257, 5000])
def test_wide_projection_plan(libs, n):
    """The benchmark's `wide` plan: every lane of a wave meets the same group
    of (returnflag, linestatus) far more often than Q1's five sums suggest --
    seven sums and a count per row."""
    oracle, product = libs
    got, tiers, _ = run_plan(product, wide_plan, _tpch(n), product=True)
    assert tiers == [0]
    assert got[0] == _oracle(oracle, ("wide", n), wide_plan, _tpch(n))


# ---- bound key/value chunks -------------------------------------------------

KV_TYPES = [GX_TYPE_I64, GX_TYPE_DECIMAL, GX_TYPE_DECIMAL]
KV_FRACS = [0, 0, 0]


def kv_plan(lib, grouped=True):
    """group by k: sum(v), min(v), max(v), count(w), count(*). w is nullable,
    so the counts cannot be shared (sharedCnt off)."""
    b = P.Builder(lib)
    src = b.source(KV_TYPES, KV_FRACS)
    k = b.colref(0, GX_TYPE_I64)
    v = b.colref(1, GX_TYPE_DECIMAL, 0)
    w = b.colref(2, GX_TYPE_DECIMAL, 0)
    aggs = [(GX_AGG_SUM, v, 0), (GX_AGG_MIN, v, 0), (GX_AGG_MAX, v, 0),
            (GX_AGG_COUNT, w, 0), (GX_AGG_COUNT, -1, 0)]
    agg = b.hashagg(src, [k] if grouped else [], aggs)
    out_types = ([GX_TYPE_I64] if grouped else []) + \
        [GX_TYPE_DECIMAL] * 3 + [GX_TYPE_I64] * 2
    return b, src, agg, out_types, [0] * len(out_types)


def kv_chunk(lib, rows):
    from tidb_amd.chunkpy import PyChunk
    from tidb_amd.decimals import str_to_decimal_bytes
    memo = {}

    def d(s):
        if s is None:
            return None
        if s not in memo:
            memo[s] = str_to_decimal_bytes(lib, s)
        return memo[s]
    chunk = PyChunk(KV_TYPES, len(rows), KV_FRACS)
    for k, v, w in rows:
        chunk.append_row([k, d(v), d(w)])
    return chunk


def _kv_bind(rows):
    return lambda lib: (lambda ex, src: ex.bind_chunks(src,
                                                       [kv_chunk(lib, rows)]))


def ndv_rows(ndv, n=5000):
    """n rows over exactly `ndv` keys, every key in every block's 250 rows
    (ndv <= 250) or spread evenly; small signed values, every third w NULL."""
    return [(i % ndv, str((i * 7) % 1000 - 500),
             None if i % 3 == 0 else str(i % 11)) for i in range(n)]


def test_tier_boundaries(libs):
    """S, S+1, 64, 65 and ~2000 distinct keys -> tiers 0, 1, 1, 2, 2; the
    second open goes straight to the sticky tier and returns the same rows."""
    oracle, product = libs
    # S comes from the engine, not from this file
    _, _, S = run_plan(product, kv_plan, _kv_bind(ndv_rows(2, 64))(product),
                       product=True)
    assert 2 <= S < 64
    for ndv, tier in [(S, 0), (S + 1, 1), (64, 1), (65, 2), (2000, 2)]:
        rows = ndv_rows(ndv)
        got, tiers, _ = run_plan(product, kv_plan, _kv_bind(rows)(product),
                                 opens=2, product=True)
        want = _oracle(oracle, ("kv", ndv), kv_plan, _kv_bind(rows)(oracle))
        assert tiers == [tier, tier], (ndv, tiers)
        assert len(want) == ndv
        assert got[0] == want and got[1] == want, ndv


BIG = "900000000000000000"  # 9 x 10^17: decimal(18,0), 75 of them pass 2^64


def carry_rows(groups, sign):
    """600 rows of +-9e17: every copy's accLo wraps and carries into accHi
    (hi = -1 path for the negative ones). NULL keys form a group of their
    own; w is NULL on every fourth row."""
    rows = []
    for i in range(600):
        neg = {"pos": False, "neg": True, "mixed": (i * 7) % 3 == 0}[sign]
        k = None if (groups > 1 and i % 50 == 0) else i % groups
        rows.append((k, ("-" if neg else "") + BIG,
                     None if i % 4 == 0 else "1"))
    return rows


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "force_wide"])
@pytest.mark.parametrize("sign", ["pos", "neg", "mixed"])
@pytest.mark.parametrize("groups", [1, 3])
def test_carries_across_copies(libs, monkeypatch, groups, sign, wide):
    oracle, product = libs
    rows = carry_rows(groups, sign)
    want = _oracle(oracle, ("carry", groups, sign), kv_plan,
                   _kv_bind(rows)(oracle))
    if wide:
        monkeypatch.setenv("GX_FORCE_WIDE", "1")
    got, tiers, _ = run_plan(product, kv_plan, _kv_bind(rows)(product),
                             product=True)
    assert tiers == [0]
    assert len(want) == (1 if groups == 1 else groups + 1)
    assert got[0] == want
