"""Decimal units columns: a resident table's consumed decimal
columns are converted once at bind to int64 units at the declared frac, and
the fused scan / join-agg probe read those 8 B/row instead of the 40 B
MyDecimal stream. Results must stay exactly the oracle's; every case also
asserts on gx_debug_dec_units_cols, so none can pass on the 40 B fallback.
"""
import ctypes
import struct

import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_AGG_SUM, GX_F_LT, GX_TPCH_CUSTOMER,
                         GX_TPCH_LINEITEM, GX_TPCH_ORDERS, GX_TYPE_DECIMAL,
                         GX_TYPE_I64, GX_TYPE_STRING, load_oracle,
                         load_product)
from tidb_amd import plan as P

pytestmark = pytest.mark.gpu

# wave (64), block (256) and 2-deep-pipeline (512) edges of a 256-thread block
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 513, 5000]


@pytest.fixture(scope="module")
def libs():
    return load_oracle(), load_product()


def _units_cols(lib, ex):
    """Columns the executor serves from a units column (product engine only)."""
    lib.gx_debug_dec_units_cols.restype = ctypes.c_int32
    lib.gx_debug_dec_units_cols.argtypes = [ctypes.c_void_p]
    return lib.gx_debug_dec_units_cols(ex.ex)


def _as_map(rows):
    return {(r[0], r[1]): tuple(r[2:]) for r in rows}


def _q1(lib, bind, opens=1, count=False):
    """Q1 over whatever `bind(ex, src)` binds; `opens` open/pull/close cycles
    on ONE executor. Returns ([result map per cycle], units-column count)."""
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
        n_units = _units_cols(lib, ex) if count else None
    finally:
        ex.free()
        b.free()
    return results, n_units


def _tpch(n):
    return lambda ex, src: ex.bind_tpch(src, GX_TPCH_LINEITEM, n)


_oracle_q1 = {}


def _oracle_q1_tpch(oracle, n):
    if n not in _oracle_q1:  # one oracle run per size, shared by every case
        _oracle_q1[n] = _q1(oracle, _tpch(n))[0][0]
    return _oracle_q1[n]


@pytest.mark.parametrize("jit", [True, False], ids=["jit", "interpreted"])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_q1_edge_sizes(libs, monkeypatch, n, jit):
    oracle, product = libs
    if not jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    opens = 2 if n == 5000 else 1
    got, n_units = _q1(product, _tpch(n), opens=opens, count=True)
    assert n_units == 4
    want = _oracle_q1_tpch(oracle, n)
    for g in got:  # a re-open reads the same units columns: identical rows
        assert g == want


def test_jit_source_has_no_parse(libs):
    """Once the columns are compacted the generated kernel loads units and
    holds no decimal parse at all."""
    _, product = libs
    product.gx_debug_jit_source.restype = ctypes.c_char_p
    product.gx_debug_jit_source.argtypes = [ctypes.c_void_p]
    b, src, agg, out_types, out_fracs = P.q1_plan(product)
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, 5000)
    before = product.gx_debug_jit_source(ex.ex).decode()
    ex.open()
    ex.pull_all(out_types, out_fracs,
                data_caps=[2048 if t == 4 else None for t in out_types])
    ex.close()
    after = product.gx_debug_jit_source(ex.ex).decode()
    n_units = _units_cols(product, ex)
    ex.free()
    b.free()
    assert n_units == 4
    assert before.count("parseDecimalRaw<WIDE>(raw.get(") == 4
    assert "parseDecimalRaw" not in after and "row * 40" not in after
    assert after.count(".units)[row]") == 4


def test_switch_off(libs, monkeypatch):
    oracle, product = libs
    monkeypatch.setenv("GX_NO_DEC_UNITS", "1")
    got, n_units = _q1(product, _tpch(5000), count=True)
    assert n_units == 0
    assert got[0] == _oracle_q1_tpch(oracle, 5000)


def test_budget_keeps_40b_form(libs, monkeypatch):
    """GX_HBM_BUDGET above the table but below table + units columns: nothing
    is built and the results are unchanged."""
    oracle, product = libs
    n = 5000
    # resident lineitem by schema: i64 8 + 4 decimals x 40 + 2 char(1) strings
    # x (8 offsets + 1 byte) + time 8 = 194 B/row -> 970,000 B; the four units
    # columns add 4 x 8 B/row = 160,000 B. Half of that on top of the table
    # holds the table (no out-of-core streaming) but not the units columns.
    table = n * (8 + 4 * 40 + 2 * 9 + 8)
    units = n * 4 * 8
    assert (table, units) == (970000, 160000)
    monkeypatch.setenv("GX_HBM_BUDGET", str(table + units // 2))
    got, n_units = _q1(product, _tpch(n), count=True)
    assert n_units == 0
    assert got[0] == _oracle_q1_tpch(oracle, n)


def _chunk(lib, rows, patch=None):
    from tidb_amd.chunkpy import PyChunk
    from tidb_amd.decimals import str_to_decimal_bytes
    d = lambda s: None if s is None else (
        s if isinstance(s, bytes) else str_to_decimal_bytes(lib, s))
    date = lambda ymd: None if ymd is None else lib.gx_time_from_date(*ymd)
    chunk = PyChunk(P.LINEITEM_TYPES, len(rows), P.LINEITEM_FRACS,
                    data_caps=[None] * 5 + [64, 64] + [None])
    for (k, q, p, disc, tax, rf, ls, sd) in rows:
        chunk.append_row([k, d(q), d(p), d(disc), d(tax), rf, ls, date(sd)])
    return chunk


# the six-row table of test_q1_bound_chunks_with_nulls, with negative values
# and a NULL in EACH decimal column
NULL_ROWS = [
    (1, "10.00", "100.00", "0.05", "0.02", "A", "F", (1995, 1, 1)),
    (2, None, "-200.00", "0.00", "0.01", "A", "F", (1995, 1, 2)),
    (3, "-5.25", None, "0.10", "0.00", "A", "F", (1995, 1, 3)),
    (4, "7.00", "50.00", "0.01", None, "N", "O", (1999, 1, 1)),
    (5, "3.00", "-5.25", None, "0.03", "R", "F", (1996, 5, 5)),
    (6, "2.00", "20.00", "0.02", "-0.04", "R", "F", None),
]


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "force_wide"])
def test_bound_chunks_with_nulls(libs, monkeypatch, wide):
    """NULL rows are exempt from the proof and stay NULL; negative units
    sign-extend into the int128 VM under GX_FORCE_WIDE."""
    oracle, product = libs
    want = _q1(oracle, lambda ex, src: ex.bind_chunks(
        src, [_chunk(oracle, NULL_ROWS)]))[0][0]
    if wide:
        monkeypatch.setenv("GX_FORCE_WIDE", "1")
    got, n_units = _q1(product, lambda ex, src: ex.bind_chunks(
        src, [_chunk(product, NULL_ROWS)]), count=True)
    assert n_units == 4
    assert got[0] == want


def _outcome(lib, rows, count=False):
    """(result map | error text, units-column count): a rejected input must
    be rejected the same way with the feature on and off."""
    try:
        got, n_units = _q1(lib, lambda ex, src: ex.bind_chunks(
            src, [_chunk(lib, rows)]), count=count)
        return got[0], n_units
    except AssertionError as e:
        return "error: " + str(e), None


def _short_frac_tax(lib):
    """0.5 stored with digitsFrac 1 in the frac-2 l_tax column."""
    from tidb_amd.decimals import decimal_bytes_to_parts, str_to_decimal_bytes
    raw = bytearray(str_to_decimal_bytes(lib, "0.5"))
    if decimal_bytes_to_parts(bytes(raw))[1] != 1:  # FromString padded it
        struct.pack_into("b", raw, 1, 1)
        struct.pack_into("<i", raw, 4 + 4 * ((raw[0] + 8) // 9), 500000000)
    digits_int, digits_frac, _rf, neg, words = decimal_bytes_to_parts(bytes(raw))
    assert digits_frac == 1 and not neg
    assert words[(digits_int + 8) // 9] == 500000000
    return bytes(raw)


FALLBACK_BASE = [
    (1, "10.00", "100.00", "0.05", "0.02", "A", "F", (1995, 1, 1)),
    (2, "4.00", "200.00", "0.00", "0.01", "A", "F", (1995, 1, 2)),
    (3, "7.00", "50.00", "0.01", "0.08", "N", "O", (1996, 1, 1)),
]


@pytest.mark.parametrize("case", ["short_frac_tax", "wide_extendedprice"])
def test_fallback_per_column(libs, monkeypatch, case):
    """One column fails the proof (row frac != declared frac; units beyond
    int64): it alone keeps the 40 B path, the other three are compacted, and
    the outcome is the switched-off engine's."""
    oracle, product = libs

    def rows(lib):
        r = [list(x) for x in FALLBACK_BASE]
        if case == "short_frac_tax":
            r[1][P.L_TAX] = _short_frac_tax(lib)
        else:
            r[1][P.L_EXTPRICE] = "999999999999999999.99"
        return [tuple(x) for x in r]

    got, n_units = _outcome(product, rows(product), count=True)
    monkeypatch.setenv("GX_NO_DEC_UNITS", "1")
    off, n_off = _outcome(product, rows(product), count=True)
    monkeypatch.delenv("GX_NO_DEC_UNITS")
    assert got == off
    if not isinstance(off, str):
        assert (n_units, n_off) == (3, 0)
        assert got == _outcome(oracle, rows(oracle))[0]


def _dec(lib, s):
    out = (ctypes.c_uint8 * 40)()
    assert lib.gx_dec_from_string(s.encode(), len(s.encode()), out) == 0
    return bytes(out)


def _run_dec_pred(lib, n, count=False):
    """sum(l_extendedprice) where l_quantity < 24.00 (fused, no group key)."""
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    cond = b.call(GX_F_LT, GX_TYPE_I64, 0,
                  b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                  b.const_dec(_dec(lib, "24.00")))
    sel = b.selection(src, [cond])
    agg = b.hashagg(sel, [], [(GX_AGG_SUM,
                               b.colref(P.L_EXTPRICE, GX_TYPE_DECIMAL, 2), 2)])
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
    ex.open()
    rows = ex.pull_all([GX_TYPE_DECIMAL], [2])
    ex.close()
    n_units = _units_cols(lib, ex) if count else None
    ex.free()
    b.free()
    return rows, n_units


@pytest.mark.parametrize("jit", [True, False], ids=["jit", "interpreted"])
def test_decimal_predicate(libs, monkeypatch, jit):
    oracle, product = libs
    want = _run_dec_pred(oracle, 1000)[0]
    if not jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    got, n_units = _run_dec_pred(product, 1000, count=True)
    assert n_units == 2  # the predicate column and the summed column
    assert len(want) == 1 and got == want


def _run_groupby(lib, n, count=False):
    """The wide-key group-by plan of the benchmark's groupby query: group by
    (returnflag, linestatus, quantity), sum(quantity), count(*)."""
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    groups = [b.colref(P.L_RETFLAG, GX_TYPE_STRING),
              b.colref(P.L_LINESTATUS, GX_TYPE_STRING),
              b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2)]
    agg = b.hashagg(src, groups,
                    [(GX_AGG_SUM, b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2),
                      2), (GX_AGG_COUNT, -1, 0)])
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, n)
    ex.open()
    out_types = [GX_TYPE_STRING, GX_TYPE_STRING, GX_TYPE_DECIMAL,
                 GX_TYPE_DECIMAL, GX_TYPE_I64]
    rows = ex.pull_all(out_types, [0, 0, 2, 2, 0],
                       data_caps=[4096, 4096, None, None, None])
    ex.close()
    n_units = _units_cols(lib, ex) if count else None
    ex.free()
    b.free()
    return sorted(rows), n_units


def test_decimal_group_key(libs):
    oracle, product = libs
    want = _run_groupby(oracle, 1000)[0]
    got, n_units = _run_groupby(product, 1000, count=True)
    assert n_units >= 1
    assert len(want) > 1 and got == want


def test_q3_probe(libs):
    """The join-agg probe loads l_extendedprice and l_discount from units
    columns; sizes as in test_q3_parity."""
    oracle, product = libs
    import tests.test_oracle_q3 as q3
    b, (cust, orders, li), topn, out_types, out_fracs = P.q3_plan(product)
    ex = b.build(topn)
    ex.bind_tpch(cust, GX_TPCH_CUSTOMER, q3.N_CUST)
    ex.bind_tpch(orders, GX_TPCH_ORDERS, q3.N_ORD)
    ex.bind_tpch(li, GX_TPCH_LINEITEM, q3.N_LI)
    got = []
    for _ in range(2):  # the second open re-reads the resident units columns
        ex.open()
        got.append(ex.pull_all(out_types, out_fracs, data_caps=[None] * 4))
        ex.close()
    n_units = _units_cols(product, ex)
    ex.free()
    b.free()
    want = q3.run_q3(oracle)
    assert n_units >= 2
    assert len(want) > 0 and got[0] == want and got[1] == want
