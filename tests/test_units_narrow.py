"""Narrowed units columns and K rows per lane: a resident
decimal column's units are kept at the narrowest of 1/2/4/8 bytes that holds
their proven range, and the generated fused kernel gives a lane K consecutive
rows per load. Results must stay exactly the oracle's; every case asserts on
the debug width / rows-per-lane functions, so none can pass on a fallback.
"""
import ctypes

import pytest

from tests.gxlib import (GX_AGG_SUM, GX_TPCH_CUSTOMER, GX_TPCH_LINEITEM,
                         GX_TPCH_ORDERS, GX_TYPE_DECIMAL, GX_TYPE_I64,
                         load_oracle, load_product)
from tests.nullslots import POISON_MODES, fill_null_slots
from tidb_amd import plan as P

pytestmark = pytest.mark.gpu

DEC_COLS = (P.L_QUANTITY, P.L_EXTPRICE, P.L_DISCOUNT, P.L_TAX)
DEFAULT_K = 4  # rows per lane the generated kernel ships with


@pytest.fixture(scope="module")
def libs():
    return load_oracle(), load_product()


def _debug(lib, ex):
    """(widths of the four lineitem decimals, rows per lane)."""
    lib.gx_debug_dec_units_width.restype = ctypes.c_int32
    lib.gx_debug_dec_units_width.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.gx_debug_rows_per_lane.restype = ctypes.c_int32
    lib.gx_debug_rows_per_lane.argtypes = [ctypes.c_void_p]
    lib.gx_debug_lds_tier.restype = ctypes.c_int32
    lib.gx_debug_lds_tier.argtypes = [ctypes.c_void_p]
    k = lib.gx_debug_rows_per_lane(ex.ex)
    if k > 1:  # only a generated kernel on its first LDS tier reports K > 1
        assert lib.gx_debug_lds_tier(ex.ex) == 0
    return (tuple(lib.gx_debug_dec_units_width(ex.ex, c) for c in DEC_COLS), k)


def _as_map(rows):
    return {(r[0], r[1]): tuple(r[2:]) for r in rows}


def _q1(lib, bind, opens=1, debug=False):
    """Q1 over whatever `bind(ex, src)` binds. Returns ([result map per
    open], (widths, rows per lane) | None)."""
    b, src, agg, out_types, out_fracs = P.q1_plan(lib)
    ex = b.build(agg)
    bind(ex, src)
    caps = [2048 if t == 4 else None for t in out_types]
    results = []
    try:
        for _ in range(opens):
            ex.open()
            results.append(_as_map(ex.pull_all(out_types, out_fracs,
                                               data_caps=caps)))
            ex.close()
        dbg = _debug(lib, ex) if debug else None
    finally:
        ex.free()
        b.free()
    return results, dbg


def _tpch(n):
    return lambda ex, src: ex.bind_tpch(src, GX_TPCH_LINEITEM, n)


_oracle_q1 = {}


def _oracle_q1_tpch(oracle, n):
    if n not in _oracle_q1:  # one oracle run per size, shared by every case
        _oracle_q1[n] = _q1(oracle, _tpch(n))[0][0]
    return _oracle_q1[n]


def _chunk(lib, rows, str_cap=64):
    from tidb_amd.chunkpy import PyChunk
    from tidb_amd.decimals import str_to_decimal_bytes
    d = lambda s: None if s is None else str_to_decimal_bytes(lib, s)
    date = lambda ymd: None if ymd is None else lib.gx_time_from_date(*ymd)
    chunk = PyChunk(P.LINEITEM_TYPES, len(rows), P.LINEITEM_FRACS,
                    data_caps=[None] * 5 + [str_cap, str_cap] + [None])
    for (k, q, p, disc, tax, rf, ls, sd) in rows:
        chunk.append_row([k, d(q), d(p), d(disc), d(tax), rf, ls, date(sd)])
    return chunk


def _bind_rows(lib, rows, mode="zero", str_cap=64):
    def bind(ex, src):
        ch = _chunk(lib, rows, str_cap)
        fill_null_slots(ch, mode)
        ex.bind_chunks(src, [ch])
    return bind


# ---- 1. width boundaries ----

def _units_str(u):
    s = "%d.%02d" % (abs(u) // 100, abs(u) % 100)
    return "-" + s if u < 0 else s


# extreme units -> width. -128 takes two bytes: the one-byte class is
# [-127, 127] (gx_units.h); the wider classes use their full range.
BOUNDARY = [(127, 1), (128, 2), (-128, 2), (-129, 2), (32767, 2), (32768, 4),
            (-32768, 2), (-32769, 4), (2**31 - 1, 4), (2**31, 8),
            (-2**31, 4), (-2**31 - 1, 8)]


def test_units_strings():
    assert [_units_str(u) for u, _ in BOUNDARY[:5]] == [
        "1.27", "1.28", "-1.28", "-1.29", "327.67"]
    assert _units_str(2**31 - 1) == "21474836.47"
    assert _units_str(2**31) == "21474836.48"


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "force_wide"])
@pytest.mark.parametrize("extreme,width", BOUNDARY,
                         ids=[str(u) for u, _ in BOUNDARY])
def test_width_boundaries(libs, monkeypatch, extreme, width, wide):
    """l_extendedprice holds one extreme value among small ones of both
    signs; the sums under GX_FORCE_WIDE check the sign extension."""
    oracle, product = libs
    rows = [
        (1, "1.00", _units_str(extreme), "0.05", "0.02", "A", "F", (1995, 1, 1)),
        (2, "2.00", "1.00", "0.00", "0.01", "A", "F", (1995, 1, 2)),
        (3, "3.00", "-1.00", "0.10", "0.00", "A", "F", (1995, 1, 3)),
        (4, "4.00", "0.00", "0.01", "0.08", "N", "O", (1996, 1, 1)),
        (5, "5.00", _units_str(extreme), "0.02", "0.03", "N", "O", (1996, 1, 2)),
    ]
    want = _q1(oracle, _bind_rows(oracle, rows))[0][0]
    if wide:
        monkeypatch.setenv("GX_FORCE_WIDE", "1")
    got, (widths, _k) = _q1(product, _bind_rows(product, rows), debug=True)
    assert widths[1] == width
    assert got[0] == want


# ---- 2. synthetic lineitem ----

def test_synthetic_lineitem_widths(libs):
    oracle, product = libs
    got, (widths, k) = _q1(product, _tpch(5000), debug=True)
    assert widths == (2, 4, 1, 1)
    assert k == DEFAULT_K
    assert got[0] == _oracle_q1_tpch(oracle, 5000)


# ---- 3. NULLs ----

# the six-row table of test_dec_units.py: negative values and a NULL in EACH
# decimal column
NULL_ROWS = [
    (1, "10.00", "100.00", "0.05", "0.02", "A", "F", (1995, 1, 1)),
    (2, None, "-200.00", "0.00", "0.01", "A", "F", (1995, 1, 2)),
    (3, "-5.25", None, "0.10", "0.00", "A", "F", (1995, 1, 3)),
    (4, "7.00", "50.00", "0.01", None, "N", "O", (1999, 1, 1)),
    (5, "3.00", "-5.25", None, "0.03", "R", "F", (1996, 5, 5)),
    (6, "2.00", "20.00", "0.02", "-0.04", "R", "F", None),
]


@pytest.mark.parametrize("mode", POISON_MODES)
def test_nulls_poisoned(libs, mode):
    """The bytes under a NULL neither reach the result nor widen the column:
    NULL rows are exempt from the range as they are from the proof."""
    oracle, product = libs
    want = _q1(oracle, _bind_rows(oracle, NULL_ROWS))[0][0]
    zero, dz = _q1(product, _bind_rows(product, NULL_ROWS), debug=True)
    got, dp = _q1(product, _bind_rows(product, NULL_ROWS, mode), debug=True)
    # quantity -5.25..10.00 -> 2 B, price -200.00..100.00 -> 2 B,
    # discount 0..0.10 and tax -0.04..0.03 -> 1 B
    assert dz[0] == (2, 2, 1, 1) and dp[0] == dz[0]
    assert got[0] == zero[0] == want


# ---- 4. row-blocking edges ----

BLOCK_SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047,
               2048, 2049, 5000]


@pytest.mark.parametrize("mode", ["k1", "k2", "k4", "interpreted"])
@pytest.mark.parametrize("n", BLOCK_SIZES)
def test_row_blocking_edges(libs, monkeypatch, n, mode):
    oracle, product = libs
    if mode == "interpreted":
        monkeypatch.setenv("GX_NO_JIT", "1")
    else:
        monkeypatch.setenv("GX_ROWS_PER_LANE", mode[1:])
    opens = 2 if n == 5000 else 1
    got, (widths, k) = _q1(product, _tpch(n), opens=opens, debug=True)
    # a short table may not reach a column's whole range: never wider
    assert all(0 < w <= full for w, full in zip(widths, (2, 4, 1, 1)))
    # what the kernel that ran did: the interpreted one takes one row per lane
    assert k == (1 if mode == "interpreted" else int(mode[1:]))
    want = _oracle_q1_tpch(oracle, n)
    for g in got:
        assert g == want


# ---- 5. other plans ----

def _widths_of(lib, ex, cols):
    lib.gx_debug_dec_units_width.restype = ctypes.c_int32
    lib.gx_debug_dec_units_width.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    return tuple(lib.gx_debug_dec_units_width(ex.ex, c) for c in cols)


def _run_dec_pred(lib, n, debug=False):
    """sum(l_extendedprice) where l_quantity < 24.00 (fused, no group key)."""
    from tests.gxlib import GX_F_LT
    out = (ctypes.c_uint8 * 40)()
    assert lib.gx_dec_from_string(b"24.00", 5, out) == 0
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    cond = b.call(GX_F_LT, GX_TYPE_I64, 0,
                  b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                  b.const_dec(bytes(out)))
    sel = b.selection(src, [cond])
    agg = b.hashagg(sel, [], [(GX_AGG_SUM,
                               b.colref(P.L_EXTPRICE, GX_TYPE_DECIMAL, 2), 2)])
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
    ex.open()
    rows = ex.pull_all([GX_TYPE_DECIMAL], [2])
    ex.close()
    dbg = _debug(lib, ex) if debug else None
    ex.free()
    b.free()
    return rows, dbg


@pytest.mark.parametrize("jit", [True, False], ids=["jit", "interpreted"])
def test_decimal_predicate(libs, monkeypatch, jit):
    oracle, product = libs
    want = _run_dec_pred(oracle, 1000)[0]
    if not jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    got, (widths, k) = _run_dec_pred(product, 1000, debug=True)
    assert widths == (2, 4, 0, 0)  # the predicate column and the summed one
    assert k == (DEFAULT_K if jit else 1)
    assert len(want) == 1 and got == want


def test_wide_projection_plan(libs):
    from tests.test_wide_projection import wide_plan
    oracle, product = libs

    def run(lib, debug):
        b, src, agg, out_types, out_fracs = wide_plan(lib)
        ex = b.build(agg)
        ex.bind_tpch(src, GX_TPCH_LINEITEM, 1000)
        ex.open()
        caps = [2048 if t == 4 else None for t in out_types]
        rows = ex.pull_all(out_types, out_fracs, data_caps=caps)
        ex.close()
        dbg = _debug(lib, ex) if debug else None
        ex.free()
        b.free()
        return sorted(rows), dbg

    got, (widths, k) = run(product, True)
    assert widths == (2, 4, 1, 1)
    assert k == DEFAULT_K
    assert got == run(oracle, False)[0]


def test_q3_probe_reads_narrow_units(libs):
    """The join-agg probe reads l_extendedprice (4 B) and l_discount (1 B)
    at use; sizes as in test_oracle_q3."""
    oracle, product = libs
    import tests.test_oracle_q3 as q3
    b, (cust, orders, li), topn, out_types, out_fracs = P.q3_plan(product)
    ex = b.build(topn)
    ex.bind_tpch(cust, GX_TPCH_CUSTOMER, q3.N_CUST)
    ex.bind_tpch(orders, GX_TPCH_ORDERS, q3.N_ORD)
    ex.bind_tpch(li, GX_TPCH_LINEITEM, q3.N_LI)
    got = []
    for _ in range(2):
        ex.open()
        got.append(ex.pull_all(out_types, out_fracs, data_caps=[None] * 4))
        ex.close()
    widths = _widths_of(product, ex, (P.L_EXTPRICE, P.L_DISCOUNT))
    ex.free()
    b.free()
    want = q3.run_q3(oracle)
    assert widths == (4, 1)
    assert len(want) > 0 and got[0] == want and got[1] == want


def test_varlen_string_key_keeps_one_row_per_lane(libs):
    """A var-len string group key needs the offsets pair: that plan keeps the
    one-row loop, and still reads narrowed units."""
    oracle, product = libs
    flags = ["A", "AB", "ABC", "ABCD", "R"]
    rows = [(i, "%d.00" % (i % 50), "%d.25" % (i * 7 % 900), "0.0%d" % (i % 10),
             "0.0%d" % (i % 9), flags[i % 5], "F" if i % 2 else "O",
             (1995, 1 + i % 12, 1 + i % 28)) for i in range(300)]
    want = _q1(oracle, _bind_rows(oracle, rows, str_cap=4096))[0][0]
    got, (widths, k) = _q1(product, _bind_rows(product, rows, str_cap=4096),
                           debug=True)
    assert k == 1
    assert widths == (2, 4, 1, 1)
    assert len(want) > 4 and got[0] == want


# ---- 6. switches ----

def test_switch_no_units_narrow(libs, monkeypatch):
    oracle, product = libs
    monkeypatch.setenv("GX_NO_UNITS_NARROW", "1")
    got, (widths, k) = _q1(product, _tpch(5000), debug=True)
    assert widths == (8, 8, 8, 8)
    assert k == DEFAULT_K  # 8 B units have a blocked form too
    assert got[0] == _oracle_q1_tpch(oracle, 5000)

