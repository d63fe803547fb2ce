"""No result may depend on the bytes under a NULL.

Every chunk the rest of the suite binds comes from PyChunk, which leaves
00..00 under a NULL. The reference's Column.AppendNull leaves the previous
value there, and the engine uploads bound chunks verbatim, so a kernel that
reads a slot without looking at the bitmap passes everywhere else and is
wrong on real chunks. Here each scenario runs with the NULL slots of its
fixed-width columns rewritten (tests/nullslots.py: stale / ones / extreme /
random) and must give what the zero-filled run gives:

  CPU:  oracle(S, mode) == oracle(S, zero), and oracle(S, zero) == a Python
        model where one is cheap (the sorts, the packed group-by);
  GPU:  product(S, mode) == oracle(S, zero), no error raised.

Rows compare exactly (integers, times, decimals digit for digit, strings,
None for NULL); f64 sums within the suite's f64 tolerance (tests/README.md);
rows of undefined order are sorted with the (x is None, x) key on both
sides. A mode changes the data only, never the plan. Every scenario asserts
at least 8 rewritten slots in each nullable column it relies on.

Sites: the device sort (bare source, TopN slice, above a left outer join,
above a Selection), fused aggregation (packed and wide group keys, every
aggregate, an expression plan; generated, interpreted and int128 kernels),
Selection, Projection, the hash join (one, two and general keys, all eight
join types, other-conditions, partitioned).

The join-aggregate (Q3-class) pipeline runs through the chunk-bound builder
of test_joinagg_general.py with NULLs in its join keys and in the ship
date. Its group slots hold the build payloads (order date, ship priority)
without a NULL flag. The plan's filter on the order date drops that
column's NULL rows before they reach a slot; a NULL ship priority used to
come back as the bytes under it (as 0 from a zero-filled chunk), and is now
refused at open.
"""
import ctypes
import functools
import math
from decimal import Decimal

import numpy as np
import pytest

from tests.gxlib import (GX_AGG_AVG, GX_AGG_COUNT, GX_AGG_COUNT_DISTINCT,
                         GX_AGG_FIRSTROW, GX_AGG_MAX, GX_AGG_MIN, GX_AGG_SUM,
                         GX_F_CAST_DEC, GX_F_CAST_INT, GX_F_GREATEST, GX_F_GT,
                         GX_F_HOUR, GX_F_IF, GX_F_IFNULL, GX_F_IS_NOT_NULL,
                         GX_F_IS_NULL, GX_F_LEAST, GX_F_LIKE_PREFIX, GX_F_LT,
                         GX_F_MONTH, GX_F_MUL, GX_F_OR, GX_F_PLUS, GX_F_ROUND,
                         GX_F_YEAR, GX_TYPE_DECIMAL, GX_TYPE_F64, GX_TYPE_I64,
                         GX_TYPE_STRING, GX_TYPE_TIME, load_oracle,
                         load_product)
from tests.nullslots import POISON_MODES, count_null_slots, fill_null_slots
from tests.test_expr_fuzz import null_order_key
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk
from tidb_amd.plan import GX_F_LIKE

I64, F64, DEC, TIME, STR = (GX_TYPE_I64, GX_TYPE_F64, GX_TYPE_DECIMAL,
                            GX_TYPE_TIME, GX_TYPE_STRING)
P_NULL = 0.25
WIDE_RETRY = "narrow overflow -> wide retry"


def _date(y, m, d):
    return (y << 50) | (m << 46) | (d << 41) | 0xE  # fspTt 0b1110: TypeDate


def _datetime(y, m, d, h, mi, s):
    return (y << 50) | (m << 46) | (d << 41) | (h << 36) | (mi << 30) | (s << 24)


class Scn:
    """tables: [(types, fracs, rows)], decimals as strings, times as raw u64.
    plan(b, lib, srcs, is_oracle) -> (root, out_types, out_fracs).
    nullable: [(table, column)] the scenario relies on."""

    def __init__(self, name, tables, plan, nullable, ordered=False, env=None,
                 f64=None):
        self.name, self.tables, self.plan = name, tables, plan
        self.nullable, self.ordered = nullable, ordered
        self.env = env or {}
        self.f64 = f64  # {sum column: count column} / {avg column: None}


_DEC40 = {}


def _dec40(lib, s):
    key = (lib._name, s)
    if key not in _DEC40:
        out = (ctypes.c_uint8 * 40)()
        assert lib.gx_dec_from_string(s.encode(), len(s.encode()), out) == 0
        _DEC40[key] = bytes(out)
    return _DEC40[key]


def _chunk(lib, types, fracs, rows):
    ch = PyChunk(types, max(len(rows), 1), fracs,
                 [len(rows) * 16 + 16 if t == STR else None for t in types])
    for r in rows:
        ch.append_row([_dec40(lib, v) if t == DEC and v is not None else v
                       for v, t in zip(r, types)])
    return ch


ROW_KEY = lambda r: tuple((x is None, x) for x in r)


def pull_cycles(ex, out_types, out_fracs, data_caps, opens):
    """opens open/pull/close cycles on one executor; the rows of each. After
    the first, one more cycle is opened, pulled for a single chunk and
    closed, so the next one starts from a half-drained run."""
    out = []
    for cycle in range(opens):
        if cycle == 1:
            ex.open()
            ex.pull_one(out_types, out_fracs, data_caps=data_caps)
            ex.close()
        ex.open()
        out.append(ex.pull_all(out_types, out_fracs, data_caps=data_caps))
        ex.close()
    return out


def _run(lib, scn, mode, is_oracle, opens=None):
    """opens=None: the rows of one open. opens=k: a list of k row lists, one
    per open/pull/close cycle on the same executor (pull_cycles)."""
    b = P.Builder(lib)
    srcs = [b.source(t, f) for t, f, _ in scn.tables]
    root, out_types, out_fracs = scn.plan(b, lib, srcs, is_oracle)
    ex = b.build(root)
    chunks = []
    for ti, (types, fracs, rows) in enumerate(scn.tables):
        ch = _chunk(lib, types, fracs, rows)
        n = fill_null_slots(ch, mode, seed=ti + 1)
        fixed = [c for c, t in enumerate(types) if t != STR]
        assert n == (0 if mode == "zero"
                     else sum(count_null_slots(ch, c) for c in fixed))
        for t2, c in scn.nullable:
            if t2 == ti:  # a scenario that poisons nothing proves nothing
                assert count_null_slots(ch, c) >= 8, (scn.name, ti, c)
        chunks.append(ch)
        ex.bind_chunks(srcs[ti], [ch])
    cycles = pull_cycles(ex, out_types, out_fracs,
                         [1 << 16 if t == STR else None for t in out_types],
                         opens or 1)
    ex.free()
    b.free()
    if not scn.ordered:
        cycles = [sorted(rows, key=ROW_KEY) for rows in cycles]
    return cycles[0] if opens is None else cycles


_WANT = {}


def _want(scn):
    """oracle(S, zero), computed once per scenario."""
    if scn.name not in _WANT:
        _WANT[scn.name] = _run(load_oracle(), scn, "zero", True)
    return _WANT[scn.name]


F64_TOL = lambda ref, n: 1e-12 * max(abs(ref), 1.0) * math.sqrt(max(n, 1))


def _assert_same(got, want, scn):
    if not scn.f64:
        assert got == want, scn.name
        return
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for c, (gv, wv) in enumerate(zip(g, w)):
            if c not in scn.f64 or wv is None or gv is None:
                assert gv == wv, (scn.name, c, g, w)
            else:  # a sum over at most w[count column] values, as
                # test_float_aggs counts them; an avg is one division
                cnt = scn.f64[c]
                n = 1 if cnt is None else w[cnt]
                assert abs(gv - wv) <= F64_TOL(wv, n), (scn.name, c, g, w)


def _check_oracle(scn, mode):
    assert len(_want(scn)) > 0
    assert _run(load_oracle(), scn, mode, True) == _want(scn)  # bit-exact


def _check_product(scn, mode, monkeypatch, opens=None):
    """opens=k: k cycles on one executor, each equal to the oracle's single
    open."""
    monkeypatch.setenv("GX_DEBUG", "1")
    for var in ("GX_NO_JIT", "GX_FORCE_WIDE", "GX_GLDS", "GX_HBM_BUDGET",
                "GX_SORT_RUN_ROWS"):
        if var in scn.env:
            monkeypatch.setenv(var, scn.env[var])
        else:
            monkeypatch.delenv(var, raising=False)
    got = _run(load_product(), scn, mode, False, opens)
    for rows in [got] if opens is None else got:
        _assert_same(rows, _want(scn), scn)


def _maybe(rng, v):
    return None if rng.random() < P_NULL else v


# ------------------------------------------------------------------ sort ---

SORT_VALS = {
    I64: [-2, -1, 0, 1, 2],
    TIME: [_date(1994, 1, 5), _date(1994, 1, 6), _datetime(1995, 7, 1, 0, 0, 0),
           _datetime(1995, 7, 1, 12, 0, 1), _date(1998, 12, 31)],
    DEC: ["-10.50", "-0.01", "0.00", "0.01", "7.25"],
}
SORT_NUM = {I64: lambda v: v, TIME: lambda v: v & ~0xF, DEC: Decimal}
SORT_TYPES = {"i64": I64, "time": TIME, "dec": DEC}
DIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@functools.lru_cache(maxsize=None)
def _sort_rows(typ, n):
    """(a, b, id): a and b nullable over 5 and 4 values, so ties are common;
    id unique, so the order is total."""
    rng = np.random.default_rng(1000 * typ + n)
    ids = rng.permutation(n)
    vals = SORT_VALS[typ]
    return [(_maybe(rng, vals[int(rng.integers(0, 5))]),
             _maybe(rng, vals[int(rng.integers(0, 4))]), int(ids[i]))
            for i in range(n)]


@functools.lru_cache(maxsize=None)
def _sort_scn(tname, n, desc, limit=-1, offset=0):
    typ = SORT_TYPES[tname]
    types = [typ, typ, I64]
    fracs = [2, 2, 0] if typ == DEC else [0, 0, 0]

    def plan(b, lib, srcs, is_oracle):
        keys = [b.colref(c, types[c], fracs[c]) for c in range(3)]
        return (b.topn(srcs[0], keys, list(desc) + [0], limit, offset),
                types, fracs)

    return Scn(f"sort-{tname}-{n}-{desc}-{limit}-{offset}",
               [(types, fracs, _sort_rows(typ, n))], plan, [(0, 0), (0, 1)],
               ordered=True)


def _sort_model(tname, n, desc, limit=-1, offset=0):
    num = SORT_NUM[SORT_TYPES[tname]]
    key = lambda r: null_order_key(
        [None if v is None else num(v) for v in r[:2]] + [r[2]],
        list(desc) + [0])
    rows = sorted(_sort_rows(SORT_TYPES[tname], n), key=key)
    return rows[offset:] if limit < 0 else rows[offset:offset + limit]


SORT_NS = [65, 1025, 5000]


@pytest.mark.parametrize("n", SORT_NS)
@pytest.mark.parametrize("tname", list(SORT_TYPES))
def test_oracle_sort_model(tname, n):
    for desc in DIRS:
        assert _want(_sort_scn(tname, n, desc)) == _sort_model(tname, n, desc)
    assert _want(_sort_scn(tname, n, (0, 1), 100, 13)) == \
        _sort_model(tname, n, (0, 1), 100, 13)


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("n", SORT_NS)
@pytest.mark.parametrize("tname", list(SORT_TYPES))
def test_oracle_sort(tname, n, mode):
    for desc in DIRS:
        _check_oracle(_sort_scn(tname, n, desc), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("n", SORT_NS)
@pytest.mark.parametrize("tname", list(SORT_TYPES))
def test_sort(tname, n, mode, monkeypatch):
    """runDeviceSort over a bare source, ORDER BY a, b, id in the four
    asc/desc combinations of (a, b)."""
    for desc in DIRS:
        _check_product(_sort_scn(tname, n, desc), mode, monkeypatch)


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("tname", list(SORT_TYPES))
def test_oracle_topn_slice(tname, mode):
    for desc in ((0, 1), (1, 0)):
        _check_oracle(_sort_scn(tname, 1025, desc, 100, 13), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("tname", list(SORT_TYPES))
def test_topn_slice(tname, mode, monkeypatch):
    """LIMIT 100 OFFSET 13: the offset is no multiple of 8, so the emission
    repacks the gathered null bitmaps."""
    for desc in ((0, 1), (1, 0)):
        _check_product(_sort_scn(tname, 1025, desc, 100, 13), mode,
                       monkeypatch)


@functools.lru_cache(maxsize=None)
def _join_sort_scn(desc, limit=1000, offset=0):
    """ORDER BY (build payload, probe payload, id) above a left outer join
    (test_join_types._run_outer_sorted's shape): the first key is NULL both
    where the build row held a NULL and where the join null-extended."""
    rng = np.random.default_rng(41)
    brows = [(k, _maybe(rng, int(rng.integers(0, 5)))) for k in range(150)]
    prows = [(_maybe(rng, int(rng.integers(0, 220))),
              _maybe(rng, int(rng.integers(0, 4))), i) for i in range(600)]

    def plan(b, lib, srcs, is_oracle):
        j = b.hashjoin(srcs[0], srcs[1], [b.colref(0, I64)],
                       [b.colref(0, I64)], join_type=1)
        keys = [b.colref(c, I64) for c in (1, 3, 4)]
        return (b.topn(j, keys, [desc, desc, 0], limit, offset), [I64] * 5,
                [0] * 5)

    tag = "" if (limit, offset) == (1000, 0) else f"-{limit}-{offset}"
    return Scn(f"join-sort-{desc}{tag}",
               [([I64] * 2, [0] * 2, brows), ([I64] * 3, [0] * 3, prows)],
               plan, [(0, 1), (1, 0), (1, 1)], ordered=True)


@functools.lru_cache(maxsize=None)
def _sel_sort_scn(desc, limit=100, offset=0):
    """TopN above a Selection (test_selection's topn shape): c > 2 drops
    the rows whose c is NULL, then ORDER BY a, b, id LIMIT 100."""
    rng = np.random.default_rng(43)
    types, fracs = [I64, DEC, I64, I64], [0, 2, 0, 0]
    rows = [(_maybe(rng, int(rng.integers(-2, 3))),
             _maybe(rng, SORT_VALS[DEC][int(rng.integers(0, 5))]), i,
             _maybe(rng, int(rng.integers(0, 10)))) for i in range(900)]

    def plan(b, lib, srcs, is_oracle):
        sel = b.selection(srcs[0], [b.call(GX_F_GT, I64, 0, b.colref(3, I64),
                                           b.const_i64(2))])
        keys = [b.colref(c, types[c], fracs[c]) for c in (0, 1, 2)]
        return (b.topn(sel, keys, [desc, 1 - desc, 0], limit, offset), types,
                fracs)

    tag = "" if (limit, offset) == (100, 0) else f"-{limit}-{offset}"
    return Scn(f"sel-sort-{desc}{tag}", [(types, fracs, rows)], plan,
               [(0, 0), (0, 1), (0, 3)], ordered=True)


ABOVE = {"join": _join_sort_scn, "selection": _sel_sort_scn}


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("below", list(ABOVE))
def test_oracle_sort_above(below, mode):
    for desc in (0, 1):
        scn = ABOVE[below](desc)
        assert len(_want(scn)) >= 100
        _check_oracle(scn, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("below", list(ABOVE))
def test_sort_above(below, mode, monkeypatch):
    for desc in (0, 1):
        _check_product(ABOVE[below](desc), mode, monkeypatch)


# ----------------------------------------------------- fused aggregation ---

# columns: g small key, w key >= 2^31, gd decimal key, gt time key,
# d dec(.,2), k i64, f f64, e dec(.,4), c dec(.,0)
AG, AW, AGD, AGT, AD, AK, AF, AE, AC = range(9)
AGG_TYPES = [I64, I64, DEC, TIME, DEC, I64, F64, DEC, DEC]
AGG_FRACS = [0, 0, 2, 0, 2, 0, 0, 4, 0]
AGG_N = 1500


@functools.lru_cache(maxsize=None)
def _agg_rows():
    rng = np.random.default_rng(47)

    def dec(hi, frac):
        s = f"{'-' if rng.random() < 0.5 else ''}{int(rng.integers(0, hi))}"
        return s + (f".{int(rng.integers(0, 10 ** frac)):0{frac}d}"
                    if frac else "")

    rows = []
    for _ in range(AGG_N):
        rows.append((
            _maybe(rng, int(rng.integers(0, 6))),
            _maybe(rng, (1 << 31) + int(rng.integers(0, 4)) * (1 << 33)),
            _maybe(rng, ["-1.50", "0.00", "2.25"][int(rng.integers(0, 3))]),
            _maybe(rng, SORT_VALS[TIME][int(rng.integers(0, 3))]),
            _maybe(rng, dec(1000, 2)),
            _maybe(rng, int(rng.integers(-1000, 1001))),
            _maybe(rng, float(rng.standard_normal() * 100.0)),
            _maybe(rng, dec(1000, 4)),
            _maybe(rng, dec(50, 0))))
    return rows


def _agg_plan_packed(b, src):
    d, k = b.colref(AD, DEC, 2), b.colref(AK, I64)
    g = b.colref(AG, I64)
    # sum(i64) is sum(cast(k as decimal)), as the reference plans it: its
    # sum takes decimal or float arguments only, and so does the oracle's
    aggs = [(GX_AGG_SUM, d, 2), (GX_AGG_AVG, d, 6),
            (GX_AGG_SUM, b.call(GX_F_CAST_DEC, DEC, 0, k), 0),
            (GX_AGG_MIN, k, 0), (GX_AGG_MAX, d, 2), (GX_AGG_COUNT, d, 0),
            (GX_AGG_COUNT, k, 0), (GX_AGG_FIRSTROW, g, 0),
            (GX_AGG_COUNT, -1, 0)]
    return (b.hashagg(src, [g], aggs),
            [I64, DEC, DEC, DEC, I64, DEC, I64, I64, I64, I64],
            [0, 2, 6, 0, 0, 2, 0, 0, 0, 0])


def _agg_plan_f64(b, src):
    f = b.colref(AF, F64)
    aggs = [(GX_AGG_SUM, f, 0), (GX_AGG_AVG, f, 0), (GX_AGG_COUNT, -1, 0)]
    return (b.hashagg(src, [b.colref(AG, I64)], aggs),
            [I64, F64, F64, I64], [0] * 4)


def _agg_plan_distinct(b, src):
    aggs = [(GX_AGG_COUNT_DISTINCT, b.colref(AK, I64), 0)]
    return b.hashagg(src, [b.colref(AG, I64)], aggs), [I64, I64], [0, 0]


def _agg_plan_wide(b, src):
    d, k = b.colref(AD, DEC, 2), b.colref(AK, I64)
    keys = [b.colref(AW, I64), b.colref(AGD, DEC, 2), b.colref(AGT, TIME)]
    aggs = [(GX_AGG_SUM, d, 2), (GX_AGG_COUNT, k, 0), (GX_AGG_MIN, k, 0),
            (GX_AGG_MAX, d, 2), (GX_AGG_AVG, d, 6),
            (GX_AGG_FIRSTROW, keys[0], 0), (GX_AGG_COUNT, -1, 0)]
    return (b.hashagg(src, keys, aggs),
            [I64, DEC, TIME, DEC, I64, I64, DEC, DEC, I64, I64],
            [0, 2, 0, 2, 0, 0, 2, 6, 0, 0])


def _agg_plan_wide_distinct(b, src):
    keys = [b.colref(AW, I64), b.colref(AGD, DEC, 2), b.colref(AGT, TIME)]
    aggs = [(GX_AGG_COUNT_DISTINCT, b.colref(AK, I64), 0)]
    return b.hashagg(src, keys, aggs), [I64, DEC, TIME, I64], [0, 2, 0, 0]


def _agg_plan_expr(b, src):
    """sum(d * e + c), sum(IFNULL(d, c)), sum(IF(k > 0, d, c)) WHERE e IS
    NOT NULL GROUP BY g. (The device VM has no IS NULL in value context, so
    it sits in the fused filter.)"""
    d, e, c = b.colref(AD, DEC, 2), b.colref(AE, DEC, 4), b.colref(AC, DEC, 0)
    k = b.colref(AK, I64)
    mad = b.call(GX_F_PLUS, DEC, 6, b.call(GX_F_MUL, DEC, 6, d, e), c)
    ifnull = b.call(GX_F_IFNULL, DEC, 2, d, c)
    ifgt = b.call(GX_F_IF, DEC, 2,
                  b.call(GX_F_GT, I64, 0, k, b.const_i64(0)), d, c)
    aggs = [(GX_AGG_SUM, mad, 6), (GX_AGG_SUM, ifnull, 2),
            (GX_AGG_SUM, ifgt, 2)]
    sel = b.selection(src, [b.call(GX_F_IS_NOT_NULL, I64, 0, e)])
    return (b.hashagg(sel, [b.colref(AG, I64)], aggs),
            [I64, DEC, DEC, DEC], [0, 6, 2, 2])


AGG_PLANS = {
    # name: (plan, columns relied on, f64 columns)
    "packed": (_agg_plan_packed, [AG, AD, AK], None),
    "f64": (_agg_plan_f64, [AG, AF], {1: 3, 2: None}),  # n: count(*)
    "distinct": (_agg_plan_distinct, [AG, AK], None),
    "wide": (_agg_plan_wide, [AW, AGD, AGT, AD, AK], None),
    "wide-distinct": (_agg_plan_wide_distinct, [AW, AGD, AGT, AK], None),
    "expr": (_agg_plan_expr, [AG, AD, AE, AC, AK], None),
}
AGG_GENERATED = ("packed", "distinct", "expr")  # the generator takes these
AGG_ENVS = {"jit": {}, "nojit": {"GX_NO_JIT": "1"},
            "forcewide": {"GX_FORCE_WIDE": "1"}}


@functools.lru_cache(maxsize=None)
def _agg_scn(pname, ename="jit"):
    fn, cols, f64 = AGG_PLANS[pname]
    scn = Scn(f"agg-{pname}", [(AGG_TYPES, AGG_FRACS, _agg_rows())],
              lambda b, lib, srcs, is_oracle: fn(b, srcs[0]),
              [(0, c) for c in cols], env=AGG_ENVS[ename], f64=f64)
    return scn


def test_oracle_agg_packed_model():
    """sum / count / min / max of the packed plan against exact Python."""
    groups = {}
    for r in _agg_rows():
        st = groups.setdefault(r[AG], {"s": Decimal(0), "dc": 0, "ks": 0,
                                       "kc": 0, "mn": None, "mx": None,
                                       "n": 0})
        st["n"] += 1
        if r[AD] is not None:
            v = Decimal(r[AD])
            st["s"] += v
            st["dc"] += 1
            st["mx"] = v if st["mx"] is None else max(st["mx"], v)
        if r[AK] is not None:
            st["ks"] += r[AK]
            st["kc"] += 1
            st["mn"] = r[AK] if st["mn"] is None else min(st["mn"], r[AK])
    got = _want(_agg_scn("packed"))
    assert len(got) == len(groups) == 7  # six values and the NULL group
    for g, s, _avg, ks, mn, mx, dc, kc, first, n in got:
        st = groups[g]
        assert first == g
        assert (Decimal(s), Decimal(ks), mn, Decimal(mx), dc, kc, n) == \
            (st["s"], st["ks"], st["mn"], st["mx"], st["dc"], st["kc"],
             st["n"])


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("pname", list(AGG_PLANS))
def test_oracle_agg(pname, mode):
    _check_oracle(_agg_scn(pname), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("ename", list(AGG_ENVS))
@pytest.mark.parametrize("pname", list(AGG_PLANS))
def test_agg(pname, ename, mode, monkeypatch, capfd):
    """The generated kernel, the interpreter (GX_NO_JIT) and the int128 VM
    (GX_FORCE_WIDE). The non-NULL data fit int64: a slot under a NULL must
    not cost the narrow kernels a second, wide pass."""
    capfd.readouterr()
    _check_product(_agg_scn(pname, ename), mode, monkeypatch)
    log = capfd.readouterr().err
    assert "[gx] useGlds=" in log  # the engine did write its GX_DEBUG lines
    if ename == "nojit":
        assert "[gx] jit" not in log
    if ename != "forcewide":
        assert WIDE_RETRY not in log
    if ename == "jit" and pname in AGG_GENERATED:
        assert "[gx] jit ok" in log


# ------------------------------------------------- selection, projection ---

# columns: i, t, d dec(.,2), j, s string, id, e and e2 dec(.,4)
SI, ST, SD, SJ, SS, SID, SE, SE2 = range(8)
SEL_TYPES = [I64, TIME, DEC, I64, STR, I64, DEC, DEC]
SEL_FRACS = [0, 0, 2, 0, 0, 0, 4, 4]
SEL_WORDS = ["", "a", "ab", "abc", "abacus", "b", "zab", "Ab"]


@functools.lru_cache(maxsize=None)
def _sel_rows():
    rng = np.random.default_rng(53)
    dec4 = lambda: (f"{'-' if rng.random() < 0.5 else ''}"
                    f"{int(rng.integers(0, 5))}."
                    f"{int(rng.integers(0, 10 ** 4)):04d}")
    rows = []
    for i in range(700):
        rows.append((
            _maybe(rng, int(rng.integers(-5, 6))),
            _maybe(rng, _datetime(int(rng.integers(1993, 1998)),
                                  int(rng.integers(1, 13)),
                                  int(rng.integers(1, 29)),
                                  int(rng.integers(0, 24)),
                                  int(rng.integers(0, 60)),
                                  int(rng.integers(0, 60)))),
            _maybe(rng, f"{'-' if rng.random() < 0.5 else ''}"
                        f"{int(rng.integers(0, 5))}."
                        f"{int(rng.integers(0, 100)):02d}"),
            _maybe(rng, int(rng.integers(-5, 6))),
            _maybe(rng, SEL_WORDS[int(rng.integers(0, len(SEL_WORDS)))]),
            i, _maybe(rng, dec4()), _maybe(rng, dec4())))
    return rows


def _sel_conds(name, b, lib, is_oracle):
    i, j = b.colref(SI, I64), b.colref(SJ, I64)
    t, d = b.colref(ST, TIME), b.colref(SD, DEC, 2)
    cmp = lambda f, x, y: b.call(f, I64, 0, x, y)
    if name == "i64":
        return [cmp(GX_F_GT, i, b.const_i64(-2))]
    if name == "time":
        return [cmp(GX_F_GT, t, b.const_time(_date(1995, 3, 15)))]
    if name == "dec":
        return [cmp(GX_F_LT, d, b.const_dec(_dec40(lib, "1.00")))]
    if name == "colcol":
        return [cmp(GX_F_LT, i, j)]
    if name == "or":
        return [b.call(GX_F_OR, I64, 0,
                       b.call(GX_F_OR, I64, 0,
                              cmp(GX_F_LT, i, b.const_i64(-3)),
                              cmp(GX_F_GT, d, b.const_dec(_dec40(lib, "2.00")))),
                       cmp(GX_F_GT, j, b.const_i64(3)))]
    if name == "isnull":
        return [b.call(GX_F_IS_NULL, I64, 0, i),
                b.call(GX_F_IS_NOT_NULL, I64, 0, d)]
    assert name == "like"  # the oracle spells 'a%' as its prefix LIKE
    s = b.colref(SS, STR)
    like = (b.call(GX_F_LIKE_PREFIX, I64, 0, s, b.const_str("a")) if is_oracle
            else b.call(GX_F_LIKE, I64, 0, s, b.const_str("a%")))
    return [like, cmp(GX_F_GT, i, b.const_i64(-2))]


SEL_CASES = {"i64": [SI], "time": [ST], "dec": [SD], "colcol": [SI, SJ],
             "or": [SI, SD, SJ], "isnull": [SI, SD], "like": [SI]}


@functools.lru_cache(maxsize=None)
def _sel_scn(name):
    def plan(b, lib, srcs, is_oracle):
        return (b.selection(srcs[0], _sel_conds(name, b, lib, is_oracle)),
                SEL_TYPES, SEL_FRACS)

    # every column is emitted, so every nullable one counts
    return Scn(f"sel-{name}", [(SEL_TYPES, SEL_FRACS, _sel_rows())], plan,
               [(0, c) for c in (SI, ST, SD, SJ, SE, SE2)], ordered=True)


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("name", list(SEL_CASES))
def test_oracle_selection(name, mode):
    scn = _sel_scn(name)
    assert 20 < len(_want(scn)) < len(_sel_rows()) - 20
    _check_oracle(scn, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("name", list(SEL_CASES))
def test_selection(name, mode, monkeypatch):
    """Survivors in row order. A slot that does not parse as a decimal
    ('ones') must not surface as a bad-decimal error."""
    _check_product(_sel_scn(name), mode, monkeypatch)


def _proj_exprs(name, b):
    i, t = b.colref(SI, I64), b.colref(ST, TIME)
    d, e = b.colref(SD, DEC, 2), b.colref(SE, DEC, 4)
    if name == "arith":
        prod = b.call(GX_F_MUL, DEC, 6, d, e)
        return [(prod, DEC, 6), (b.call(GX_F_PLUS, DEC, 4, d, e), DEC, 4),
                (b.call(GX_F_ROUND, DEC, 2, prod, b.const_i64(2)), DEC, 2),
                (b.call(GX_F_CAST_DEC, DEC, 1, e), DEC, 1),
                (b.call(GX_F_CAST_INT, I64, 0, d), I64, 0),
                (b.call(GX_F_CAST_DEC, DEC, 1, i), DEC, 1)]
    if name == "time":
        return [(b.call(f, I64, 0, t), I64, 0)
                for f in (GX_F_YEAR, GX_F_MONTH, GX_F_HOUR)]
    assert name == "pick"  # operands of one frac: the result keeps it
    e2 = b.colref(SE2, DEC, 4)
    return [(b.call(GX_F_IFNULL, DEC, 4, e, e2), DEC, 4),
            (b.call(GX_F_GREATEST, DEC, 4, e, e2), DEC, 4),
            (b.call(GX_F_LEAST, DEC, 4, e, e2), DEC, 4)]


PROJ_CASES = {"arith": [SI, SD, SE], "time": [ST], "pick": [SE, SE2]}


@functools.lru_cache(maxsize=None)
def _proj_scn(name):
    def plan(b, lib, srcs, is_oracle):
        exprs = _proj_exprs(name, b)
        return (b.projection(srcs[0], [x for x, _, _ in exprs]),
                [t for _, t, _ in exprs], [f for _, _, f in exprs])

    return Scn(f"proj-{name}", [(SEL_TYPES, SEL_FRACS, _sel_rows())], plan,
               [(0, c) for c in PROJ_CASES[name]], ordered=True)


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_oracle_projection(name, mode):
    scn = _proj_scn(name)
    want = _want(scn)
    assert len(want) == len(_sel_rows())
    for c in range(len(want[0])):  # both NULL and value outputs occur
        assert 8 <= sum(r[c] is None for r in want) <= len(want) - 8
    _check_oracle(scn, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_projection(name, mode, monkeypatch):
    """Output NULLs compare as None: what the engine writes under its own
    NULLs is not constrained."""
    _check_product(_proj_scn(name), mode, monkeypatch)


# ------------------------------------------------------------- hash join ---

N_SHARED = 30  # key values 0..29 exist on both sides, whatever the seed


def _join_keys(rng, n, hi):
    """n nullable keys in [0, hi). The first N_SHARED rows hold every shared
    value; the row before a NULL holds a shared value, so in 'stale' mode
    the bytes under every NULL key are a key that exists on the other
    side."""
    keys = list(range(N_SHARED))
    while len(keys) < n:
        if rng.random() < P_NULL:
            if keys[-1] is None or keys[-1] >= N_SHARED:
                keys[-1] = int(rng.integers(0, N_SHARED))
            keys.append(None)
        else:
            keys.append(int(rng.integers(0, hi)))
    return keys


JOIN_DECS = [f"{v // 10}.{v % 10}" for v in range(60)]  # key v as v/10
JOIN_STRS = ["", "A", "A ", "xy", "BUILDING"]


@functools.lru_cache(maxsize=None)
def _join_tables(shape, build_nulls=True, empty=None):
    """build (keys.., payload), probe (keys.., payload, id); keys and
    payloads nullable. build_nulls=False drops the build rows whose first
    key is NULL; "none" also fills the NULLs of the second key column, so no
    build key column holds one; "single" is "none" with the first key of one
    build row NULL. empty="build" / "probe" leaves that side
    without rows."""
    rng = np.random.default_rng(59)
    nb, npr = 300, 900
    bk, pk = _join_keys(rng, nb, 40), _join_keys(rng, npr, 60)
    if build_nulls is not True:
        bk = [k for k in bk if k is not None]
        nb = len(bk)
        if build_nulls == "single":
            bk[nb // 2] = None
    bpay = [_maybe(rng, int(rng.integers(0, 50))) for _ in range(nb)]
    ppay = [_maybe(rng, int(rng.integers(0, 50))) for _ in range(npr)]
    if shape == "one":
        kt, kf = [I64], [0]
        b2 = lambda i: (bk[i],)
        p2 = lambda i: (pk[i],)
        fb = fp = kf
    elif shape == "two":
        kt, kf = [I64, I64], [0, 0]
        bs = [_maybe(rng, int(rng.integers(0, 2))) for _ in range(nb)]
        ps = [_maybe(rng, int(rng.integers(0, 2))) for _ in range(npr)]
        if build_nulls in ("none", "single"):
            bs = [i % 2 if v is None else v for i, v in enumerate(bs)]
        b2 = lambda i: (bk[i], bs[i])
        p2 = lambda i: (pk[i], ps[i])
        fb = fp = kf
    else:  # general: decimal key (frac 1 joins frac 2 by value) + string
        assert shape == "general"
        kt, kf = [DEC, STR], [1, 0]
        bs = [_maybe(rng, JOIN_STRS[int(rng.integers(0, 5))]) for _ in range(nb)]
        ps = [_maybe(rng, JOIN_STRS[int(rng.integers(0, 5))]) for _ in range(npr)]
        if build_nulls in ("none", "single"):
            bs = [JOIN_STRS[i % 5] if v is None else v
                  for i, v in enumerate(bs)]
        b2 = lambda i: (None if bk[i] is None else JOIN_DECS[bk[i]], bs[i])
        p2 = lambda i: (None if pk[i] is None else JOIN_DECS[pk[i]] + "0",
                        ps[i])
        fb, fp = [1, 0], [2, 0]
    brows = [b2(i) + (bpay[i],) for i in range(nb)]
    prows = [p2(i) + (ppay[i], i) for i in range(npr)]
    if empty == "build":
        brows = []
    elif empty is not None:
        assert empty == "probe"
        prows = []
    return ((kt + [I64], fb + [0], brows), (kt + [I64, I64], fp + [0, 0], prows))


@functools.lru_cache(maxsize=None)
def _join_scn(shape, jt, build_nulls=True, other=False, budget=None,
              empty=None, build_pred=False):
    """build_pred: the build side under a Selection (payload < 25), so the
    null-aware joins' valid set is what passes it."""
    (bt, bf, brows), (pt, pf, prows) = _join_tables(shape, build_nulls, empty)
    nk = len(bt) - 1

    def plan(b, lib, srcs, is_oracle):
        bside = srcs[0]
        if build_pred:
            bside = b.selection(bside, [b.call(GX_F_LT, I64, 0,
                                               b.colref(nk, I64),
                                               b.const_i64(25))])
        root = b.hashjoin(bside, srcs[1],
                          [b.colref(c, bt[c], bf[c]) for c in range(nk)],
                          [b.colref(c, pt[c], pf[c]) for c in range(nk)],
                          join_type=jt)
        if other:  # build payload < probe payload AND probe payload < 40
            root = b.selection(root, [
                b.call(GX_F_LT, I64, 0, b.colref(nk, I64),
                       b.colref(len(bt) + nk, I64)),
                b.call(GX_F_LT, I64, 0, b.colref(len(bt) + nk, I64),
                       b.const_i64(40))])
        if jt in (3, 4, 5):
            return root, pt, pf
        if jt in (6, 7):
            return root, pt + [I64], pf + [0]
        return root, bt + pt, bf + pf

    fixed_keys = [c for c in range(nk) if bt[c] != STR]
    nullable = [(0, c) for c in fixed_keys if build_nulls is True] + \
        [(1, c) for c in fixed_keys] + [(0, nk), (1, nk)]
    nullable = [(t, c) for t, c in nullable
                if t != {"build": 0, "probe": 1}.get(empty)]
    env = {} if budget is None else {"GX_HBM_BUDGET": str(budget)}
    tag = (f"-empty-{empty}" if empty else "") + ("-pred" if build_pred else "")
    return Scn(f"join-{shape}-{jt}-{build_nulls}-{other}{tag}",
               [(bt, bf, brows), (pt, pf, prows)], plan, nullable, env=env)


def test_join_tables_shape():
    """What the join scenarios rely on: under every NULL i64 key, 'stale'
    leaves a key that the other side holds."""
    (_, _, brows), (_, _, prows) = _join_tables("one")
    for mine, other in ((brows, prows), (prows, brows)):
        there = {r[0] for r in other if r[0] is not None}
        prev = None
        n_null = 0
        for r in mine:
            if r[0] is None:
                assert prev in there
                n_null += 1
            else:
                prev = r[0]
        assert n_null >= 8
    # the null-aware joins' answer changes if a NULL is taken for a value
    assert _want(_join_scn("one", 5)) == []
    assert len(_want(_join_scn("one", 5, build_nulls=False))) > 20
    assert any(r[-1] is None for r in _want(_join_scn("one", 7, False)))


JOIN_SHAPES = ["one", "two", "general"]


def _join_scns(shape):
    scns = [_join_scn(shape, jt) for jt in range(8)]
    scns += [_join_scn(shape, jt, build_nulls=False) for jt in (5, 7)]
    scns.append(_join_scn(shape, 0, other=True))
    return scns


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("shape", JOIN_SHAPES)
def test_oracle_join(shape, mode):
    for scn in _join_scns(shape):
        assert _run(load_oracle(), scn, mode, True) == _want(scn), scn.name
    assert len(_want(_join_scn(shape, 0))) > 100
    assert len(_want(_join_scn(shape, 0, other=True))) > 20


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("shape", JOIN_SHAPES)
def test_join(shape, mode, monkeypatch):
    """All eight join types, the null-aware ones also without NULL build
    keys, and an inner join under other-conditions over the nullable
    payloads."""
    for scn in _join_scns(shape):
        _check_product(scn, mode, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("jt", [1, 4])
def test_join_partitioned(jt, mode, monkeypatch, capfd):
    """GX_HBM_BUDGET (test_join_spill's knob) partitions both sides by key
    hash: the partition hash must not read a NULL key's slot either. The
    two sides and their output take 62400 bytes by the engine's estimate,
    several times the budget."""
    capfd.readouterr()
    _check_product(_join_scn("one", jt, budget=8 << 10), mode, monkeypatch)
    assert "[gx] join spill:" in capfd.readouterr().err


# -------------------------------------------------- join-aggregate (Q3) ---

JA_NULLS = {"keys": [], "date": [(1, 2)], "prio": [(1, 2), (1, 3)]}


@functools.lru_cache(maxsize=None)
def _joinagg_data(nulls):
    """customer (custkey, segment), orders (orderkey, custkey, orderdate,
    shippriority), lineitem (orderkey, price, discount, shipdate) for
    test_joinagg_general._q3_shaped. NULLs in the join keys and the ship
    date; 'date' adds NULL order dates (a payload the plan's orderdate <
    1995-03-15 filters), 'prio' NULL ship priorities as well (a payload
    nothing filters)."""
    rng = np.random.default_rng(61)
    date = (lambda v: _maybe(rng, v)) if nulls != "keys" else (lambda v: v)
    prio = (lambda v: _maybe(rng, v)) if nulls == "prio" else (lambda v: v)
    early = [_date(1994, 1, 1), _date(1994, 5, 5), _date(1995, 2, 2),
             _date(1995, 6, 1)]  # the last fails orderdate < 1995-03-15
    custs = [(_maybe(rng, k), "BUILDING" if k % 5 else "OTHER")
             for k in range(1, 61)]
    ords = [(ok, _maybe(rng, int(rng.integers(1, 61))),
             date(early[int(rng.integers(0, 4))]),
             prio(int(rng.integers(0, 5)))) for ok in range(1, 301)]
    lis = [(_maybe(rng, int(rng.integers(1, 330))),
            f"{int(rng.integers(1, 1000))}.{int(rng.integers(0, 100)):02d}",
            f"0.{int(rng.integers(0, 11)):02d}",
            _maybe(rng, _date(1996, 6, 1) if rng.random() < 0.8
                   else _date(1994, 1, 1))) for _ in range(2000)]
    return custs, ords, lis


def _bind_joinagg(lib, mode, nulls):
    from tests.test_joinagg_general import (_cust_chunk, _li_chunk,
                                            _ord_chunk, _q3_shaped)
    custs, ords, lis = _joinagg_data(nulls)
    b, srcs, topn = _q3_shaped(lib, False, 1000)  # limit above the groups
    ex = b.build(topn)
    chunks = [_cust_chunk(custs), _ord_chunk(ords), _li_chunk(lib, lis)]
    for i, ch in enumerate(chunks):
        fill_null_slots(ch, mode, seed=i + 1)
    for t, c in [(0, 0), (1, 1), (2, 0), (2, 7)] + JA_NULLS[nulls]:
        assert count_null_slots(chunks[t], c) >= 8, (t, c)
    for src, ch in zip(srcs, chunks):
        ex.bind_chunks(src, [ch])
    return b, ex, chunks


def _run_joinagg(lib, mode, nulls):
    b, ex, _chunks = _bind_joinagg(lib, mode, nulls)
    ex.open()
    out = ex.pull_all([I64, TIME, I64, DEC], [0, 0, 0, 4])
    ex.close()
    ex.free()
    b.free()
    return sorted(out, key=ROW_KEY)


@functools.lru_cache(maxsize=None)
def _want_joinagg(nulls):
    return _run_joinagg(load_oracle(), "zero", nulls)


@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("nulls", list(JA_NULLS))
def test_oracle_joinagg(nulls, mode):
    want = _want_joinagg(nulls)
    assert 20 < len(want) < 1000
    # the filter drops NULL order dates; a NULL ship priority is a group key
    assert not any(r[1] is None for r in want)
    assert any(r[2] is None for r in want) == (nulls == "prio")
    assert _run_joinagg(load_oracle(), mode, nulls) == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", POISON_MODES)
@pytest.mark.parametrize("nulls", ["keys", "date"])
def test_joinagg(nulls, mode, monkeypatch):
    for var in ("GX_NO_JIT", "GX_FORCE_WIDE", "GX_GLDS", "GX_HBM_BUDGET"):
        monkeypatch.delenv(var, raising=False)
    assert _run_joinagg(load_product(), mode, nulls) == _want_joinagg(nulls)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["zero", "stale"])
def test_joinagg_null_payload_refused(mode):
    """A NULL ship priority reaches the pipeline's group slots, which have
    no NULL flag: the query fails with a descriptive error instead of
    handing the slot's bytes back as a value."""
    lib = load_product()
    b, ex, _chunks = _bind_joinagg(lib, mode, "prio")
    rc = lib.gx_open(ex.ex)
    n = ctypes.c_int32(0)
    if rc == 0:
        out = PyChunk([I64, TIME, I64, DEC], 1024, [0, 0, 0, 4])  # owns g's
        g = out.as_gx()                                          # buffers
        rc = lib.gx_next(ex.ex, ctypes.byref(g), ctypes.byref(n))
    err = ex.error()
    ex.close()
    ex.free()
    b.free()
    assert rc != 0 and n.value == 0
    assert "nullable build payload column" in err
