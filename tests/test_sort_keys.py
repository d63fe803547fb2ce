"""The device sort's key domain beyond TPC-H's.

test_full_sort and test_edge_cases sort generator lineitem rows: positive
values, decimals stored at the column's frac, no NULLs. Here chunk-bound
sources carry what the key compose (sortComposeKeysKernel) and the pass
bounds (beginBit / endBit from the OR and AND of all keys) never saw:
the int64 extremes, keys that differ in bit 63 or in bit 0 only, all-equal
keys (the skipped value pass, with and without the null pass after it),
negative decimals, -0.0000, decimals stored with fewer frac digits than the
column's (the scale-up branch), times that differ only in the 4 tag bits,
every byte value as a dense char(1) key, keys that differ in bits 4..63
only over more than 1024 rows (a begin bit other than 0 with an end bit of
64, where rocPRIM's merge-sort compare mask overflows its shift; the engine
now starts such passes at bit 0), and row counts around the 1024-row
emission boundary.

A unique last key makes every order total. CPU: oracle == Python model
(NULL first ascending, last descending). GPU: product == oracle, exactly.

char(1): the reference compares utf8mb4_bin PAD SPACE, that is after
trimming trailing spaces, so ' ' is the empty string and sorts below
'\\x01'. The oracle's string compare and the kernel's ' ' -> 0 mapping both
do exactly that; neither side needed a fix.
"""
import ctypes
import functools
from decimal import Decimal

import numpy as np
import pytest

from tests.gxlib import (GX_TYPE_DECIMAL, GX_TYPE_I64, GX_TYPE_STRING,
                         GX_TYPE_TIME, load_oracle, load_product)
from tests.test_expr_fuzz import null_order_key
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk

I64, DEC, TIME, STR = GX_TYPE_I64, GX_TYPE_DECIMAL, GX_TYPE_TIME, GX_TYPE_STRING
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _dec40(lib, s):
    out = (ctypes.c_uint8 * 40)()
    assert lib.gx_dec_from_string(s.encode(), len(s.encode()), out) == 0
    return bytes(out)


def _executor(lib, ktype, kfrac, rows, desc):
    """ORDER BY key [desc], id over a bound (key, id) chunk."""
    types, fracs = [ktype, I64], [kfrac, 0]
    b = P.Builder(lib)
    src = b.source(types, fracs)
    root = b.sort(src, [b.colref(0, ktype, kfrac), b.colref(1, I64)],
                  [desc, 0])
    ex = b.build(root)
    ch = PyChunk(types, max(len(rows), 1), fracs,
                 [len(rows) + 16 if ktype == STR else None, None])
    for k, i in rows:
        ch.append_row([_dec40(lib, k) if ktype == DEC and k is not None
                       else k, i])
    ex.bind_chunks(src, [ch])
    return b, ex, types, fracs


def _sorted_by(lib, ktype, kfrac, rows, desc):
    b, ex, types, fracs = _executor(lib, ktype, kfrac, rows, desc)
    ex.open()
    out = ex.pull_all(types, fracs,
                      data_caps=[1 << 14 if ktype == STR else None, None])
    ex.close()
    ex.free()
    b.free()
    return out


def _shuffled(keys, seed):
    """(key, unique id) rows in a seeded random order."""
    rng = np.random.default_rng(seed)
    return [(keys[j], int(i)) for i, j in enumerate(rng.permutation(len(keys)))]


def _with_nulls(keys):
    return [None if i % 4 == 1 else k for i, k in enumerate(keys)]


TIME_BASE = (1996 << 50) | (2 << 46) | (29 << 41) | (23 << 36) | (59 << 30)

I64_KEYS = {
    "extremes": [INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1,
                 INT64_MAX] * 10,
    "equal": [5] * 100,
    "equal-nullable": _with_nulls([5] * 100),  # no value pass, a null pass
    "signbit": [5, 5 + INT64_MIN] * 40,
    "bit0": [6, 7] * 40,
}
# decimal(20,4) appended with 0, 2 and 4 frac digits; -0.0000 ties with zero
DEC_KEYS = ["-12345.6789", "-0.0001", "0.0000", "-0.0000", "0", "0.00", "3",
            "3.00", "3.0000", "2.5", "2.50", "-7", "-7.25", "-7.2500",
            "1234567890123.4567", "-1234567890123.4567", "99999999999999",
            "0.01", "0.0100", "-0.01"] * 4
# equal after & ~0xF, so equal keys: the tag bits must not order them
TIME_KEYS = [TIME_BASE | t for t in (0x0, 0x2, 0x7, 0xE, 0xF)] * 12 + \
    [TIME_BASE + (1 << 24), TIME_BASE - (1 << 24), (1 << 41) | 0xE] * 6
CHAR_KEYS = [bytes([v]) for v in range(1, 256)] * 2


def _wide_keys(n=1500):
    """Keys that differ in bits 4..63 (time: 4..62) and in none below: many
    radix passes from a begin bit other than 0, over more than one block of
    rows. i64: random multiples of 16 over the whole range; time: years
    1..8191 (pulled times read back as int64, so bit 63 stays clear) down
    to the microsecond (bits 4..23)."""
    rng = np.random.default_rng(11)
    i64 = [int(v) & ~0xF for v in
           rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64)]
    time = [(int(rng.integers(1, 8192)) << 50) |
            (int(rng.integers(1, 13)) << 46) | (int(rng.integers(1, 29)) << 41) |
            (int(rng.integers(0, 24)) << 36) | (int(rng.integers(0, 60)) << 30) |
            (int(rng.integers(0, 60)) << 24) |
            (int(rng.integers(0, 10 ** 6)) << 4) for _ in range(n)]
    return i64, time


WIDE_I64, WIDE_TIME = _wide_keys()

CASES = {f"i64-{k}": (I64, 0, _shuffled(v, 3)) for k, v in I64_KEYS.items()}
CASES["dec"] = (DEC, 4, _shuffled(DEC_KEYS, 5))
CASES["dec-nullable"] = (DEC, 4, _shuffled(_with_nulls(DEC_KEYS), 5))
CASES["time"] = (TIME, 0, _shuffled(TIME_KEYS, 7))
CASES["time-nullable"] = (TIME, 0, _shuffled(_with_nulls(TIME_KEYS), 7))
CASES["char1"] = (STR, 0, _shuffled(CHAR_KEYS, 9))
CASES["i64-bits4to63"] = (I64, 0, _shuffled(WIDE_I64, 13))
CASES["time-micros"] = (TIME, 0, _shuffled(WIDE_TIME, 13))
CASES["time-micros-nullable"] = (TIME, 0, _shuffled(_with_nulls(WIDE_TIME), 13))


def _num(ktype, k):
    if k is None:
        return None
    if ktype == DEC:
        return Decimal(k)
    if ktype == TIME:
        return k & ~0xF
    if ktype == STR:  # PAD SPACE; bytes order as their first byte, '' as -1
        return k.rstrip(b" ")[0] if k.rstrip(b" ") else -1
    return k


def _model_ids(ktype, rows, desc):
    key = lambda r: null_order_key([_num(ktype, r[0]), r[1]], [desc, 0])
    return [i for _, i in sorted(rows, key=key)]


@functools.lru_cache(maxsize=None)
def _want(case, desc):
    ktype, kfrac, rows = CASES[case]
    return _sorted_by(load_oracle(), ktype, kfrac, rows, desc)


def _check_rows_kept(ktype, rows, out):
    """The sort moved whole rows: each id still carries its key."""
    by_id = {i: k for k, i in rows}
    assert len(out) == len(rows)
    for k, i in out:
        if ktype == STR:  # pulled strings decode lossily above 0x7F
            want = by_id[i]
            assert k == want.decode("utf8", "replace")
        elif ktype == DEC:
            assert (k is None) == (by_id[i] is None)
            assert k is None or Decimal(k) == Decimal(by_id[i])
        else:
            assert k == by_id[i]


@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_sort_keys(case, desc):
    ktype, _, rows = CASES[case]
    out = _want(case, desc)
    _check_rows_kept(ktype, rows, out)
    assert [i for _, i in out] == _model_ids(ktype, rows, desc)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_sort_keys(case, desc):
    ktype, kfrac, rows = CASES[case]
    assert _sorted_by(load_product(), ktype, kfrac, rows, desc) == \
        _want(case, desc)


def test_cases_hold_what_they_claim():
    a, b = I64_KEYS["signbit"][:2]
    assert (a ^ b) & 0xFFFFFFFFFFFFFFFF == 1 << 63
    a, b = I64_KEYS["bit0"][:2]
    assert a ^ b == 1
    assert len({k & ~0xF for k in TIME_KEYS[:5]}) == 1
    assert len(set(TIME_KEYS[:5])) == 5
    assert {len(k.split(".")[1]) if "." in k else 0 for k in DEC_KEYS} == \
        {0, 1, 2, 4}
    assert b" " in CHAR_KEYS and len(set(CHAR_KEYS)) == 255
    for keys, top in ((WIDE_I64, 63), (WIDE_TIME, 62)):
        o = a = keys[0] & 0xFFFFFFFFFFFFFFFF
        for k in keys:
            o, a = o | (k & 0xFFFFFFFFFFFFFFFF), a & k
        assert (o ^ a) == (1 << (top + 1)) - 16  # bits 4..top differ
    assert sum(k is None for k in _with_nulls(DEC_KEYS)) >= 8


# ---- row counts around the 1024-row emission boundary ----

ROW_COUNTS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 5000]


@functools.lru_cache(maxsize=None)
def _count_rows(n):
    rng = np.random.default_rng(n)
    return [(None if rng.random() < 0.25 else int(rng.integers(-3, 4)), int(i))
            for i in rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def _want_count(n, desc):
    return _sorted_by(load_oracle(), I64, 0, _count_rows(n), desc)


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_oracle_sort_row_counts(n):
    rows = _count_rows(n)
    for desc in (0, 1):
        out = _want_count(n, desc)
        _check_rows_kept(I64, rows, out)
        assert [i for _, i in out] == _model_ids(I64, rows, desc)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_sort_row_counts(n):
    for desc in (0, 1):
        assert _sorted_by(load_product(), I64, 0, _count_rows(n), desc) == \
            _want_count(n, desc)


# ---- a non-NULL key past int64 units: refused, not mis-sorted ----

# 16 integer digits at frac 4: 1e20 units, past int64
OVERFLOW_ROWS = [("1.5000", 0), ("9999999999999999.9999", 1), ("-2.2500", 2)]


def test_oracle_sorts_overflowing_decimal_key():
    out = _sorted_by(load_oracle(), DEC, 4, OVERFLOW_ROWS, 0)
    assert [i for _, i in out] == [2, 0, 1]


@pytest.mark.gpu
def test_overflowing_decimal_key_refused():
    """The device sort orders decimals as int64 units at the column's frac.
    A value that does not fit fails the query with the sort-key error; no
    row comes back."""
    lib = load_product()
    b, ex, types, fracs = _executor(lib, DEC, 4, OVERFLOW_ROWS, 0)
    rc = lib.gx_open(ex.ex)
    n = ctypes.c_int32(0)
    if rc == 0:  # the sort runs at the first Next
        chunk = PyChunk(types, 1024, fracs)
        g = chunk.as_gx()
        rc = lib.gx_next(ex.ex, ctypes.byref(g), ctypes.byref(n))
    err = ex.error()
    ex.close()
    ex.free()
    b.free()
    assert rc != 0 and n.value == 0
    assert "sort key error" in err
