"""Compact result download: after the fused launch a small
kernel appends the occupied group slots to a result block whose header also
carries the pass's error flag and selected-row count, and ONE copy per open
brings it to a pinned host buffer. More than 256 groups, and wide group
keys, keep the full-table download. Every case equals the oracle run of the
same plan and asserts on gx_debug_result_compact, so none can pass on the
other path.
"""
import ctypes

import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_AGG_MODE_COMPLETE,
                         GX_AGG_MODE_PARTIAL, GX_AGG_SUM, GX_F_LT,
                         GX_TPCH_LINEITEM, GX_TYPE_DECIMAL, GX_TYPE_I64,
                         GX_TYPE_STRING, load_oracle, load_product)
from tests.test_lds_replicas import (_kv_bind, kv_plan, lds_tier, ndv_rows)
from tidb_amd import plan as P

pytestmark = pytest.mark.gpu

CAP = 256  # gxp::kResultCap


@pytest.fixture(scope="module")
def libs():
    return load_oracle(), load_product()


def used_compact(lib, ex):
    lib.gx_debug_result_compact.restype = ctypes.c_int32
    lib.gx_debug_result_compact.argtypes = [ctypes.c_void_p]
    return lib.gx_debug_result_compact(ex.ex)


def run(lib, plan, bind, product=False):
    """(sorted rows, compact?, tier) of one open/pull/close."""
    b, src, agg, out_types, out_fracs = plan(lib)
    ex = b.build(agg)
    bind(ex, src)
    caps = [4096 if t == GX_TYPE_STRING else None for t in out_types]
    try:
        ex.open()
        rows = sorted(ex.pull_all(out_types, out_fracs, data_caps=caps),
                      key=repr)
        ex.close()
        compact = used_compact(lib, ex) if product else None
        tier = lds_tier(lib, ex) if product else None
    finally:
        ex.free()
        b.free()
    return rows, compact, tier


def _li_chunk(lib, rows):
    from tidb_amd.chunkpy import PyChunk
    from tidb_amd.decimals import str_to_decimal_bytes
    chunk = PyChunk(P.LINEITEM_TYPES, len(rows), P.LINEITEM_FRACS,
                    data_caps=[None] * 5 + [64, 64] + [None])
    for (k, q, p, disc, tax, rf, ls, sd) in rows:
        d = lambda s: s if isinstance(s, bytes) else str_to_decimal_bytes(lib, s)
        chunk.append_row([k, d(q), d(p), d(disc), d(tax), rf, ls,
                          lib.gx_time_from_date(*sd)])
    return chunk


# every row is shipped after Q1's cutoff and carries quantity >= 0
LATE_ROWS = [(i, "%d.00" % (i % 7), "10.00", "0.05", "0.02", "AR"[i % 2], "F",
              (1999, 1, 1 + i % 9)) for i in range(300)]


def _dec(lib, s):
    out = (ctypes.c_uint8 * 40)()
    assert lib.gx_dec_from_string(s.encode(), len(s.encode()), out) == 0
    return bytes(out)


def ungrouped_plan(mode):
    """sum(l_extendedprice), count(*) where l_quantity < -1.00: no survivor."""
    def plan(lib):
        b = P.Builder(lib)
        src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
        cond = b.call(GX_F_LT, GX_TYPE_I64, 0,
                      b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                      b.const_dec(_dec(lib, "-1.00")))
        sel = b.selection(src, [cond])
        agg = b.hashagg(sel, [], [(GX_AGG_SUM,
                                   b.colref(P.L_EXTPRICE, GX_TYPE_DECIMAL, 2),
                                   2), (GX_AGG_COUNT, -1, 0)], mode)
        if mode == GX_AGG_MODE_PARTIAL:
            return b, src, agg, [GX_TYPE_DECIMAL, GX_TYPE_I64,
                                 GX_TYPE_I64], [2, 0, 0]
        return b, src, agg, [GX_TYPE_DECIMAL, GX_TYPE_I64], [2, 0]
    return plan


@pytest.mark.parametrize("mode", [GX_AGG_MODE_COMPLETE, GX_AGG_MODE_PARTIAL],
                         ids=["complete", "partial"])
@pytest.mark.parametrize("grouped", [True, False],
                         ids=["grouped", "ungrouped"])
def test_zero_surviving_rows(libs, grouped, mode):
    """An empty result block: the rows are whatever the oracle gives (none,
    or the one default row of an ungrouped COMPLETE aggregate)."""
    oracle, product = libs
    plan = (lambda lib: P.q1_plan(lib, mode)) if grouped else \
        ungrouped_plan(mode)
    bind = lambda lib: (lambda ex, src: ex.bind_chunks(
        src, [_li_chunk(lib, LATE_ROWS)]))
    want = run(oracle, plan, bind(oracle))[0]
    got, compact, _ = run(product, plan, bind(product), product=True)
    assert compact == 1
    assert len(want) == (1 if not grouped and
                         mode == GX_AGG_MODE_COMPLETE else 0)
    assert got == want


@pytest.mark.parametrize("ndv,compact", [(CAP - 1, 1), (CAP, 1), (CAP + 1, 0),
                                         (2000, 0)])
def test_cap_edge_and_bank_fold(libs, ndv, compact):
    """CAP-1 and CAP groups fit the block, CAP+1 falls back to the full table.
    All of them aggregate global-direct (tier 2), so the kernel folds the 16
    accumulator banks for the first two and the host folds them for the
    others -- the same fold, gxp::foldGroupSlot."""
    oracle, product = libs
    rows = ndv_rows(ndv)
    want = run(oracle, kv_plan, _kv_bind(rows)(oracle))[0]
    got, was_compact, tier = run(product, kv_plan, _kv_bind(rows)(product),
                                 product=True)
    assert (was_compact, tier) == (compact, 2)
    assert len(want) == ndv and got == want


def test_streamed_run(libs, monkeypatch):
    """A budget below the 970,000 B table streams 5000 rows in 4096-row
    slices; only the last slice compacts."""
    oracle, product = libs
    bind = lambda ex, src: ex.bind_tpch(src, GX_TPCH_LINEITEM, 5000)
    want = run(oracle, P.q1_plan, bind)[0]
    monkeypatch.setenv("GX_HBM_BUDGET", "200000")
    got, compact, tier = run(product, P.q1_plan, bind, product=True)
    assert (compact, tier) == (1, 0)
    assert len(want) >= 4 and got == want


def groupby_plan(lib):
    """Wide group keys: (returnflag, linestatus, quantity)."""
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    groups = [b.colref(P.L_RETFLAG, GX_TYPE_STRING),
              b.colref(P.L_LINESTATUS, GX_TYPE_STRING),
              b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2)]
    agg = b.hashagg(src, groups,
                    [(GX_AGG_SUM, b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                      2), (GX_AGG_COUNT, -1, 0)])
    return b, src, agg, [GX_TYPE_STRING, GX_TYPE_STRING, GX_TYPE_DECIMAL,
                         GX_TYPE_DECIMAL, GX_TYPE_I64], [0, 0, 2, 2, 0]


def test_wide_keys_keep_full_download(libs):
    oracle, product = libs
    bind = lambda ex, src: ex.bind_tpch(src, GX_TPCH_LINEITEM, 1000)
    want = run(oracle, groupby_plan, bind)[0]
    got, compact, _ = run(product, groupby_plan, bind, product=True)
    assert compact == 0
    assert len(want) > 1 and got == want


def test_error_flag_keeps_its_text(libs):
    """A row stored at frac 3 in the frac-2 l_tax column raises the scale flag
    on device (kErrScale = 4); the message is read from the block's header."""
    _, product = libs
    rows = [list(r) for r in LATE_ROWS[:100]]
    for r in rows:
        r[7] = (1995, 1, 1)  # survive the date filter
    rows[37][4] = "0.123"
    b, src, agg, out_types, out_fracs = P.q1_plan(product)
    ex = b.build(agg)
    ex.bind_chunks(src, [_li_chunk(product, [tuple(r) for r in rows])])
    try:
        ex.open()
        with pytest.raises(AssertionError) as e:
            ex.pull_all(out_types, out_fracs,
                        data_caps=[2048, 2048] + [None] * 8)
        assert ("device execution error flag 0x4 (unsupported data shape or "
                "overflow)") in str(e.value)
    finally:
        ex.free()
        b.free()
