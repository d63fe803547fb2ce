"""ORDER BY / TopN on variable-length string keys, f64 keys, and tables that
carry a varlen payload.

The device sort turns each general-varlen key into a dense rank column
(gx_strkey.h: MSD refinement over 7-byte window keys) and gathers varlen
payload through the final permutation. Chunk-bound tables with a unique last
key (id) make every order total.

CPU: oracle == Python model. The model's string key is k.rstrip(b" ")
compared as bytes (utf8mb4_bin PAD SPACE); NULL is first ascending and last
descending. GPU: product == oracle, exactly, for both directions. Pulled
strings above 0x7F decode lossily, so the checks are the id order and the
equality with the oracle's rows.

NaN is left out: the oracle orders f64 with `<`, which is no strict weak
order there, and the device key order for NaN is unspecified.
"""
import functools
import struct
import subprocess
import os

import numpy as np
import pytest

from tests.gxlib import (GX_F_GT, GX_TPCH_CUSTOMER, GX_TYPE_F64, GX_TYPE_I64,
                         GX_TYPE_STRING, load_oracle, load_product)
from tests.test_expr_fuzz import null_order_key
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk

I64, F64, STR = GX_TYPE_I64, GX_TYPE_F64, GX_TYPE_STRING
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- running a plan over chunk-bound tables ----

def _caps(types, nbytes=1 << 16):
    return [nbytes if t == STR else None for t in types]


def _run(lib, tables, plan, pulls=1):
    """tables: [(types, rows)]; plan(b, srcs) -> (root, out_types). Opens,
    pulls everything and closes `pulls` times; returns the list of results."""
    b = P.Builder(lib)
    srcs = [b.source(t) for t, _ in tables]
    root, out_types = plan(b, srcs)
    ex = b.build(root)
    chunks = []
    for (types, rows), s in zip(tables, srcs):
        nbytes = sum(len(v) for r in rows for v in r if isinstance(v, bytes))
        ch = PyChunk(types, max(len(rows), 1), None, _caps(types, nbytes + 16))
        for r in rows:
            ch.append_row(list(r))
        ex.bind_chunks(s, [ch])
        chunks.append(ch)
    outs = []
    for _ in range(pulls):
        ex.open()
        outs.append(ex.pull_all(out_types, None, data_caps=_caps(out_types)))
        ex.close()
    ex.free()
    b.free()
    return outs


def _order_by(cols, types, desc, limit=-1, offset=0):
    """plan: ORDER BY cols (desc flags) over the single source."""
    def plan(b, srcs):
        keys = [b.colref(c, types[c]) for c in cols]
        if limit < 0:
            return b.sort(srcs[0], keys, list(desc)), types
        return b.topn(srcs[0], keys, list(desc), limit, offset), types
    return plan


# ---- the model ----

def _ranks(keys):
    """bytes (or None) -> dense rank of the trimmed bytes, None kept."""
    distinct = sorted({k.rstrip(b" ") for k in keys if k is not None})
    rank = {k: i for i, k in enumerate(distinct)}
    return [None if k is None else rank[k.rstrip(b" ")] for k in keys]


def _model(rows, types, cols, desc):
    """rows sorted as the plan asks; string columns compare by _ranks."""
    num = []
    for c in cols:
        vals = [r[c] for r in rows]
        num.append(_ranks(vals) if types[c] == STR else vals)
    order = sorted(range(len(rows)),
                   key=lambda i: null_order_key([v[i] for v in num], desc))
    return [rows[i] for i in order]


def _shuffled(keys, seed):
    """(key, unique id) rows in a seeded random order."""
    rng = np.random.default_rng(seed)
    return [(keys[j], int(i)) for i, j in enumerate(rng.permutation(len(keys)))]


def _same_rows(out, want_rows, types):
    """out (pulled, strings decoded) holds want_rows (bytes) in order."""
    assert len(out) == len(want_rows)
    for got, want in zip(out, want_rows):
        for g, w, t in zip(got, want, types):
            if t == STR and w is not None:
                w = w.decode("utf8", "replace")
            assert g == w, (got, want)


# ---- (key, id) cases ----

BASE = b"abcdefghijklmnopqrstuv"  # 22 bytes
SEGMENTS = [b"AUTOMOBILE", b"BUILDING", b"FURNITURE", b"MACHINERY",
            b"HOUSEHOLD"]


def _window_edges():
    keys = [BASE[:n] for n in range(23)]
    for at in (6, 7, 13, 14):  # first difference at this byte
        keys.append(BASE[:at] + b"Z" + BASE[at + 1:])
        keys.append(BASE[:at] + b"\x01" + BASE[at + 1:])
    keys += [b"abcdefg", b"abcdefg\0", b"abcdefgh"]
    return keys * 2


def _long_prefix(n=1500):
    rng = np.random.default_rng(17)
    return [b"p" * 30 + str(int(rng.integers(0, 4000))).encode() * int(
        rng.integers(1, 3)) for _ in range(n)]


def _with_nulls(keys):
    return [None if i % 4 == 1 else k for i, k in enumerate(keys)]


STR_KEYS = {
    "window-edges": _window_edges(),
    "embedded-nul": [b"", b"\0", b"ab", b"ab\0", b"ab\0\0", b"ab\0a"] * 6,
    "pad-space": [b"ab", b"ab ", b"ab  ", b" ", b"", b"ab c", b"abcdefg",
                  b"abcdefg ", b" " * 7, b" " * 8, b"abcdefg  h"] * 4,
    "unsigned": [b"\x7f", b"\x80", b"\xff", b"a\x7f", b"a\x80", b"a\xff",
                 b"abcdefg\x7f", b"abcdefg\x80", b"abcdefg\xff",
                 b"abcdefgh\x7fz", b"abcdefgh\xffz", b"a"] * 4,
    "equal40": [b"e" * 40] * 100,
    "equal40-nullable": _with_nulls([b"e" * 40] * 100),
    "long-prefix": _long_prefix(),
    "five-values": [SEGMENTS[i % 5] for i in range(3000)],
    "nullable": _with_nulls([b"same", b"same ", b"", b"samf", b"same",
                             b"sam", b"same\0"] * 12),
}
CASES = {k: (STR, _shuffled(v, 3 + i))
         for i, (k, v) in enumerate(STR_KEYS.items())}

F64_KEYS = [-1e308, 1e308, float("-inf"), float("inf"), -0.0, 0.0, -0.0, 0.0,
            5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
            1.0, 1.0000000000000002, 0.9999999999999999, -1.0,
            -1.0000000000000002, -2.5, 2.5, 3.0] * 3


def _random_doubles(n=1500):
    rng = np.random.default_rng(23)
    bits = rng.integers(0, 1 << 63, n, dtype=np.int64) * 2 + \
        rng.integers(0, 2, n, dtype=np.int64)
    vals = [struct.unpack("<d", struct.pack("<q", int(v)))[0] for v in bits]
    return [v if v == v else float(i) for i, v in enumerate(vals)]  # no NaN


CASES["f64"] = (F64, _shuffled(F64_KEYS, 31))
CASES["f64-nullable"] = (F64, _shuffled(_with_nulls(F64_KEYS), 31))
CASES["f64-random"] = (F64, _shuffled(_random_doubles(), 37))

ROW_COUNTS = [1, 2, 63, 64, 65, 1023, 1024, 1025]
COUNT_VALUES = [b"", b" ", b"k", b"key", b"key ", b"keyword", b"keywords",
                b"keywords and more", b"keywords and mor", b"l"]


def _count_rows(n):
    rng = np.random.default_rng(n)
    return [(None if rng.random() < 0.2 else
             COUNT_VALUES[int(rng.integers(0, len(COUNT_VALUES)))], int(i))
            for i in rng.permutation(n)]


for _n in ROW_COUNTS:
    CASES[f"rows-{_n}"] = (STR, _count_rows(_n))


@functools.lru_cache(maxsize=None)
def _want(case, desc):
    ktype, rows = CASES[case]
    types = [ktype, I64]
    return _run(load_oracle(), [(types, rows)],
                _order_by([0, 1], types, [desc, 0]))[0]


@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_sort_strkeys(case, desc):
    ktype, rows = CASES[case]
    types = [ktype, I64]
    _same_rows(_want(case, desc), _model(rows, types, [0, 1], [desc, 0]),
               types)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_sort_strkeys(case, desc):
    ktype, rows = CASES[case]
    types = [ktype, I64]
    got = _run(load_product(), [(types, rows)],
               _order_by([0, 1], types, [desc, 0]))[0]
    assert got == _want(case, desc)


def test_cases_hold_what_they_claim():
    def trims(keys):
        return {k.rstrip(b" ") for k in keys if k is not None}

    def first_diff(a, b):
        return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y),
                    min(len(a), len(b)))

    we = STR_KEYS["window-edges"]
    assert {len(k) for k in we} >= set(range(23))
    for at in (6, 7, 13, 14):
        assert any(first_diff(k, BASE) == at and len(k) == len(BASE)
                   for k in we)
    assert {b"abcdefg", b"abcdefg\0", b"abcdefgh"} <= set(we)
    assert len(trims(STR_KEYS["embedded-nul"])) == 6  # NULs are data
    ps = STR_KEYS["pad-space"]
    assert {b"ab", b"ab ", b"ab  "} <= set(ps) and b"ab c" in trims(ps)
    assert {b" ", b"", b" " * 7, b" " * 8} <= set(ps)
    assert len(trims(ps)) == 5  # '', ab, 'ab c', abcdefg, 'abcdefg  h'
    assert b"abcdefg " in ps and len(b"abcdefg") == 7  # space past the edge
    us = STR_KEYS["unsigned"]
    assert {k[0] for k in us} >= {0x7F, 0x80, 0xFF}
    assert {k[8] for k in us if len(k) > 8} >= {0x7F, 0xFF}  # second window
    assert len(set(STR_KEYS["equal40"])) == 1
    assert len(STR_KEYS["equal40"][0]) == 40
    lp = STR_KEYS["long-prefix"]
    assert len(lp) > 1024 and all(k[:30] == b"p" * 30 for k in lp)
    assert len(set(lp)) > 500  # differ from byte 30 on: five windows
    fv = STR_KEYS["five-values"]
    assert len(set(fv)) == 5 and len(fv) == 3000
    nl = STR_KEYS["nullable"]
    assert b"same" in nl and b"same " in nl  # a pair tying after trim
    for name in ("equal40-nullable", "nullable"):
        assert sum(k is None for k in STR_KEYS[name]) >= 8
    assert sum(k is None for k in _with_nulls(F64_KEYS)) >= 8
    assert any(struct.pack("<d", k) == struct.pack("<d", -0.0)
               for k in F64_KEYS) and 0.0 in F64_KEYS
    a, b = struct.pack("<d", 1.0), struct.pack("<d", 1.0000000000000002)
    assert int.from_bytes(b, "little") - int.from_bytes(a, "little") == 1
    assert all(v == v for _, rows in CASES.values() for v, _ in rows
               if isinstance(v, float))  # no NaN anywhere
    assert any(k is None for k, _ in _count_rows(65))


# ---- scenarios beyond (key, id) ----

def _strs(rng, n, values):
    return [values[int(rng.integers(0, len(values)))] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _scenario(name):
    """-> (tables, plan, model rows or None, out types)."""
    rng = np.random.default_rng(53)
    vals = [b"", b"ab", b"ab ", b"abcdefg", b"abcdefgh", b"abcdefgh\0",
            b"abcdefghijklmnop", b"abcdefghijklmnoq", b"\xff", b"zz"]
    if name == "i64-str-desc":  # the rank is read through a permuted index
        types = [I64, STR, I64]
        rows = [(int(rng.integers(0, 6)), s, i)
                for i, s in enumerate(_strs(rng, 900, vals))]
        desc = [0, 1, 0]
        return ([(types, rows)], _order_by([0, 1, 2], types, desc),
                _model(rows, types, [0, 1, 2], desc), types)
    if name == "str-str-desc":  # two rank columns
        types = [STR, STR, I64]
        rows = [(s, t, i) for i, (s, t) in enumerate(
            zip(_strs(rng, 900, vals[:5]), _strs(rng, 900, vals)))]
        desc = [0, 1, 0]
        return ([(types, rows)], _order_by([0, 1, 2], types, desc),
                _model(rows, types, [0, 1, 2], desc), types)
    if name == "payload-i64-key":  # no string is compared
        types = [I64, STR, I64]
        rows = [(int(rng.integers(-40, 40)),
                 b"payload-%d" % i + b"x" * int(rng.integers(0, 20)), i)
                for i in range(1100)]
        desc = [0, 0]
        return ([(types, rows)], _order_by([0, 2], types, desc),
                _model(rows, types, [0, 2], desc), types)
    if name == "payload-str-key":
        types = [STR, STR, I64]
        rows = [(s, None if i % 5 == 2 else b"second-%d" % (i * 7), i)
                for i, s in enumerate(_strs(rng, 1100, vals))]
        desc = [1, 0]
        return ([(types, rows)], _order_by([0, 2], types, desc),
                _model(rows, types, [0, 2], desc), types)
    if name in ("topn-10-3", "topn-20-1021"):
        limit, offset = (10, 3) if name == "topn-10-3" else (20, 1021)
        types = [STR, I64]
        rows = _shuffled(STR_KEYS["long-prefix"], 59)
        desc = [0, 0]
        full = _model(rows, types, [0, 1], desc)
        return ([(types, rows)],
                _order_by([0, 1], types, desc, limit, offset),
                full[offset:offset + limit], types)
    if name == "over-selection":
        types = [STR, I64, I64]
        rows = [(s, i, int(rng.integers(0, 10)))
                for i, s in enumerate(_strs(rng, 400, vals))]

        def plan(b, srcs):
            sel = b.selection(srcs[0], [b.call(GX_F_GT, I64, 0,
                                               b.colref(2, I64),
                                               b.const_i64(2))])
            return (b.sort(sel, [b.colref(0, STR), b.colref(1, I64)], [0, 0]),
                    types)

        kept = [r for r in rows if r[2] > 2]
        return ([(types, rows)], plan, _model(kept, types, [0, 1], [0, 0]),
                types)
    if name == "over-hashjoin":
        btypes, ptypes = [I64, STR], [I64, I64]
        brows = [(k, s) for k, s in enumerate(_strs(rng, 60, vals))]
        prows = [(int(rng.integers(0, 90)), i) for i in range(400)]
        otypes = btypes + ptypes

        def plan(b, srcs):
            j = b.hashjoin(srcs[0], srcs[1], [b.colref(0, I64)],
                           [b.colref(0, I64)])
            return (b.sort(j, [b.colref(1, STR), b.colref(3, I64)], [1, 0]),
                    otypes)

        joined = [(k, brows[k][1], k, i) for k, i in prows if k < 60]
        return ([(btypes, brows), (ptypes, prows)], plan,
                _model(joined, otypes, [1, 3], [1, 0]), otypes)
    raise KeyError(name)


SCENARIOS = ["i64-str-desc", "str-str-desc", "payload-i64-key",
             "payload-str-key", "topn-10-3", "topn-20-1021", "over-selection",
             "over-hashjoin"]


@functools.lru_cache(maxsize=None)
def _want_scenario(name):
    tables, plan, _, _ = _scenario(name)
    return _run(load_oracle(), tables, plan)[0]


@pytest.mark.parametrize("name", SCENARIOS)
def test_oracle_sort_scenarios(name):
    _, _, model, types = _scenario(name)
    assert len(model) >= 10
    _same_rows(_want_scenario(name), model, types)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENARIOS)
def test_sort_scenarios(name):
    tables, plan, _, _ = _scenario(name)
    assert _run(load_product(), tables, plan)[0] == _want_scenario(name)


def test_scenarios_hold_what_they_claim():
    _, _, model, _ = _scenario("payload-str-key")
    assert sum(r[1] is None for r in model) >= 8
    assert len(_scenario("topn-20-1021")[2]) == 20
    assert len(_scenario("over-hashjoin")[2]) > 100


# ---- re-open: a bare source stays sorted; above a Selection the sort, the
# rank and the payload gather run again ----

REOPEN = ["payload-str-key", "over-selection"]


@pytest.mark.parametrize("name", REOPEN)
def test_oracle_reopen(name):
    tables, plan, _, _ = _scenario(name)
    a, b = _run(load_oracle(), tables, plan, pulls=2)
    assert a == b == _want_scenario(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REOPEN)
def test_reopen(name):
    tables, plan, _, _ = _scenario(name)
    a, b = _run(load_product(), tables, plan, pulls=2)
    assert a == b == _want_scenario(name)


# ---- the generator's customer table ----

CUSTOMER_ROWS = 5000


def _customer(lib, keys, desc):
    b = P.Builder(lib)
    src = b.source(P.CUSTOMER_TYPES)
    root = src
    if keys:
        root = b.sort(src, [b.colref(c, P.CUSTOMER_TYPES[c]) for c in keys],
                      desc)
    ex = b.build(root)
    ex.bind_tpch(src, GX_TPCH_CUSTOMER, CUSTOMER_ROWS)
    ex.open()
    out = ex.pull_all(P.CUSTOMER_TYPES, None, data_caps=[None, 1 << 16])
    ex.close()
    ex.free()
    b.free()
    return out


@functools.lru_cache(maxsize=None)
def _want_customer(desc):
    return _customer(load_oracle(), [P.C_MKTSEGMENT, P.C_CUSTKEY], [desc, 0])


@pytest.mark.parametrize("desc", [0, 1])
def test_oracle_customer_by_segment(desc):
    rows = [(k, s.encode()) for k, s in _customer(load_oracle(), [], [])]
    assert len(rows) == CUSTOMER_ROWS and len({s for _, s in rows}) == 5
    types = P.CUSTOMER_TYPES
    _same_rows(_want_customer(desc),
               _model(rows, types, [P.C_MKTSEGMENT, P.C_CUSTKEY], [desc, 0]),
               types)


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [0, 1])
def test_customer_by_segment(desc):
    got = _customer(load_product(), [P.C_MKTSEGMENT, P.C_CUSTKEY], [desc, 0])
    assert got == _want_customer(desc)


# ---- the stand-alone host check of gx_strkey.h ----

def test_strkey_check_builds_and_passes(tmp_path):
    exe = tmp_path / "strkey_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I",
                    os.path.join(REPO, "tidb_amd", "csrc"),
                    os.path.join(REPO, "tools", "strkey_check.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
