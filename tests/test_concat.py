"""CONCAT / CONCAT_WS / CAST(int AS CHAR) as outputs of the device Projection
(include/gx_executor.h GX_F_CONCAT, GX_F_CONCAT_WS, GX_F_CAST_STR).

The reference is the pure-Python model below: it works on bytes, uses
str(int) for the cast and implements the NULL rules (CONCAT: NULL if any
argument is NULL; CONCAT_WS with a constant separator: NULL arguments drop
with their separator, never NULL, '' when every argument is NULL). The
oracle does not know these codes.

CPU tests (product library, no GPU): plan acceptance and rejection, and the
host evaluator gx_debug_strcat_eval, which runs the same gx_strcat.h source
as the kernels (length pass, prefix sum, 256-row tile byte mapping).
GPU tests: the kernels against the model over the tile edges (0, 1, 255, 256,
257 rows) and three Next calls (3000 rows), NULL / empty / 70 000-byte
inputs, a dense char(1) source, a Selection below, a mixed projection and
re-open.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_F_CAST_DEC, GX_F_GT, GX_F_LENGTH,
                         GX_F_LOWER, GX_F_PLUS, GX_F_SUBSTR, GX_F_TRIM,
                         GX_F_UPPER, GX_F_YEAR, GX_TPCH_LINEITEM,
                         GX_TYPE_DECIMAL, GX_TYPE_I64, GX_TYPE_STRING,
                         GX_TYPE_TIME, load_product)
from tests.nullslots import fill_null_slots
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk
from tidb_amd.plan import (GX_F_CAST_STR, GX_F_CONCAT, GX_F_CONCAT_WS,
                           GX_F_LIKE)

TYPES = [GX_TYPE_STRING, GX_TYPE_STRING, GX_TYPE_I64, GX_TYPE_TIME]
S, I = GX_TYPE_STRING, GX_TYPE_I64

# the string set of tests/test_string_builtins.py::STRS
STRS = ["hello world", "", "A", "BUILDING", "mixed-Case-Str",
        "a-rather-long-string-beyond-sixteen-bytes", "trail  ",
        "  lead", None, "x"]
INTS = [0, -1, 9, 10, -10, 10 ** 18, 2 ** 63 - 1, -2 ** 63, None]
ROW_COUNTS = [0, 1, 255, 256, 257, 3000]


# ---------------- expressions: one tree, a plan builder and a model --------
# string: ("s", col) ("const", bytes) ("upper"|"lower"|"trim", e)
#         ("substr", e, pos, len) ("cast", int_e) ("concat", [e..])
#         ("ws", sep_bytes, [e..])
# int:    ("i", col) ("year", col) ("length", ("s", col)) ("add", a, b)
#         ("iconst", v)

def mk(b, e):
    k = e[0]
    if k == "s":
        return b.colref(e[1], S)
    if k == "const":
        return b.const_str(e[1])
    if k in ("upper", "lower", "trim"):
        f = {"upper": GX_F_UPPER, "lower": GX_F_LOWER, "trim": GX_F_TRIM}[k]
        return b.call(f, S, 0, mk(b, e[1]))
    if k == "substr":
        return b.call(GX_F_SUBSTR, S, 0, mk(b, e[1]), b.const_i64(e[2]),
                      b.const_i64(e[3]))
    if k == "cast":
        return b.call(GX_F_CAST_STR, S, 0, mk(b, e[1]))
    if k == "concat":
        return b.call(GX_F_CONCAT, S, 0, *[mk(b, a) for a in e[1]])
    if k == "ws":
        return b.call(GX_F_CONCAT_WS, S, 0, b.const_str(e[1]),
                      *[mk(b, a) for a in e[2]])
    if k == "i":
        return b.colref(e[1], I)
    if k == "iconst":
        return b.const_i64(e[1])
    if k == "year":
        return b.call(GX_F_YEAR, I, 0, b.colref(e[1], GX_TYPE_TIME))
    if k == "length":
        return b.call(GX_F_LENGTH, I, 0, mk(b, e[1]))
    if k == "add":
        return b.call(GX_F_PLUS, I, 0, mk(b, e[1]), mk(b, e[2]))
    raise AssertionError(k)


def _substr(v, pos, ln):
    start = len(v) + pos + 1 if pos < 0 else pos
    if start < 1 or start > len(v) or ln <= 0:
        return b""
    return v[start - 1:start - 1 + ln]


def ev(e, r):
    """Model value of expression e on row r = (s0, s1, i, year, time_raw):
    bytes / int, or None for NULL."""
    k = e[0]
    if k in ("s", "i"):
        return r[e[1]]
    if k in ("const", "iconst"):
        return e[1]
    if k == "year":
        return r[3]
    if k == "concat":
        parts = [ev(a, r) for a in e[1]]
        return None if any(p is None for p in parts) else b"".join(parts)
    if k == "ws":
        return e[1].join(p for p in (ev(a, r) for a in e[2]) if p is not None)
    if k == "add":
        x, y = ev(e[1], r), ev(e[2], r)
        return None if x is None or y is None else x + y
    v = ev(e[1], r)
    if v is None:
        return None
    if k == "upper":
        return bytes(c - 32 if 97 <= c <= 122 else c for c in v)
    if k == "lower":
        return bytes(c + 32 if 65 <= c <= 90 else c for c in v)
    if k == "trim":
        return v.strip(b" ")
    if k == "substr":
        return _substr(v, e[2], e[3])
    if k == "cast":
        return str(v).encode()
    if k == "length":
        return len(v)
    raise AssertionError(k)


def dec(v):
    return None if v is None else v.decode("ascii")


S0, S1, IC = ("s", 0), ("s", 1), ("i", 2)
PLANS = {
    "concat_dash": ("concat", [S0, ("const", b"-"), S1]),
    "concat_windows": ("concat", [("upper", ("trim", S0)),
                                  ("substr", S1, 2, 5), ("const", b"x")]),
    "concat_hash_int": ("concat", [("const", b"#"), ("cast", IC)]),
    "concat_year_len": ("concat", [("cast", ("year", 3)), ("const", b"/"),
                                   ("cast", ("length", S0))]),
    "concat_nested": ("concat", [S0, ("concat", [S1, ("const", b"z")])]),
    "cast_alone": ("cast", IC),
    "ws_comma": ("ws", b", ", [S0, S1, ("cast", IC)]),
    "ws_empty_sep": ("ws", b"", [S0, S1]),
}
FLAT_OF_NESTED = ("concat", [S0, S1, ("const", b"z")])
# plans the host evaluator takes: CAST_STR arguments that are plain columns
HOST_PLANS = [k for k in PLANS if k != "concat_year_len"]


# ---------------- data ----------------

@functools.lru_cache(maxsize=None)
def _rows(n, variant="base", seed=7):
    """n model rows (s0, s1, i, year, time_raw); computed once per shape."""
    lib = load_product()
    rng = np.random.default_rng(seed + n)
    rows = []
    for k in range(n):
        s0 = STRS[rng.integers(0, len(STRS))]
        s1 = STRS[rng.integers(0, len(STRS))]
        if rng.integers(0, 3) == 0:
            i = int(rng.integers(-2 ** 63, 2 ** 63 - 1))
        else:
            i = INTS[rng.integers(0, len(INTS))]
        if k < 8 and n >= 8:   # every NULL combination of (s0, s1, i)
            s0 = None if k & 1 else "a"
            s1 = None if k & 2 else ""
            i = None if k & 4 else -5
        year = None if rng.integers(0, 7) == 0 else int(rng.integers(1970, 2100))
        if variant == "s1_null":
            s1 = None
        elif variant == "empty":
            s0, s1 = "", ""
        elif variant == "long" and k == n // 2:
            s0 = "".join(chr(97 + (j * 7) % 26) for j in range(70_000))
            s1, i = "x", 10
        t = None if year is None else lib.gx_time_from_date(
            year, int(rng.integers(1, 13)), int(rng.integers(1, 29)))
        rows.append((None if s0 is None else s0.encode(),
                     None if s1 is None else s1.encode(), i, year, t))
    return tuple(rows)


def _chunks(rows):
    """Bound as <= 1000-row chunks with exact string capacities."""
    chunks = []
    for base in range(0, max(len(rows), 1), 1000):
        part = rows[base:base + 1000]
        caps = [sum(len(r[c]) for r in part if r[c] is not None) + 8
                for c in (0, 1)]
        ch = PyChunk(TYPES, max(len(part), 1), [0] * 4,
                     [caps[0], caps[1], None, None])
        for r in part:
            ch.append_row([r[0], r[1], r[2], r[4]])
        fill_null_slots(ch, "random", seed=base)  # bytes under NULLs
        chunks.append(ch)
    return chunks


def _project(exprs, rows, out_types, sel=None, opens=1, cap=1 << 18):
    """Run Projection(exprs) over [Selection(sel) ->] Source(rows) on the
    product engine; returns one row list per open."""
    lib = load_product()
    b = P.Builder(lib)
    src = b.source(TYPES)
    child = src if sel is None else b.selection(src, [sel(b)])
    ids = [mk(b, e) for e in exprs]
    ex = b.build(b.projection(child, ids))
    assert ex.error() == ""
    chunks = _chunks(rows)
    ex.bind_chunks(src, chunks)
    outs = []
    for _ in range(opens):
        ex.open()
        outs.append(ex.pull_all(out_types, [0] * len(out_types),
                                data_caps=[cap if t == S else None
                                           for t in out_types]))
        ex.close()
    ex.free()
    b.free()
    return outs


def _check_cols(got, rows, exprs):
    assert len(got) == len(rows)
    for c, e in enumerate(exprs):
        want = [ev(e, r) for r in rows]
        want = [dec(w) if isinstance(w, bytes) else w for w in want]
        have = [g[c] for g in got]
        if have != want:
            bad = next(k for k in range(len(rows)) if have[k] != want[k])
            raise AssertionError(
                f"output {c} {e}: row {bad} got {have[bad]!r:.80} "
                f"want {want[bad]!r:.80} (input {rows[bad][:3]!r:.120})")


# ---------------- CPU: plan acceptance / rejection ----------------

@pytest.mark.parametrize("name", list(PLANS) + ["over_select"])
def test_build_accepts(name):
    lib = load_product()
    b = P.Builder(lib)
    src = b.source(TYPES)
    child = src
    if name == "over_select":
        child = b.selection(src, [b.call(GX_F_GT, I, 0, b.colref(2, I),
                                         b.const_i64(0))])
        name = "ws_comma"
    ex = b.build(b.projection(child, [mk(b, PLANS[name]), b.colref(0, S)]))
    err = ex.error()
    rc = lib.gx_open(ex.ex)
    ex.free()
    b.free()
    assert err == "" and rc == 0, err


def _reject(plan_fn, *needles):
    lib = load_product()
    b = P.Builder(lib)
    src = b.source(TYPES)
    ex = b.build(plan_fn(b, src))
    rc = lib.gx_open(ex.ex)
    err = ex.error()
    ex.free()
    b.free()
    assert rc != 0, "expected a compile/open error, got rc=0"
    assert all(n in err for n in needles), err


REJECTS = {
    "nine_pieces": (("concat", [S0] * 9), ["8 pieces"]),
    "const_bytes_257": (("concat", [S0, ("const", b"x" * 257)]),
                        ["256 bytes"]),
    "const_bytes_257_with_sep": (("ws", b"," * 7, [("const", b"y" * 250), S0]),
                                 ["256 bytes"]),
    "nested_ws_in_concat": (("concat", [S0, ("ws", b",", [S0, S1])]),
                            ["CONCAT_WS nested"]),
    "nested_ws_in_ws": (("ws", b"-", [S0, ("ws", b",", [S0, S1])]),
                        ["CONCAT_WS nested"]),
    "upper_over_concat": (("upper", ("concat", [S0, S1])), ["over a CONCAT"]),
    "length_over_cast": (("length", ("cast", IC)), ["over a CONCAT"]),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_build_rejects(name):
    e, needles = REJECTS[name]
    _reject(lambda b, src: b.projection(src, [mk(b, e)]), *needles)


def test_build_rejects_column_separator():
    def plan(b, src):
        ws = b.call(GX_F_CONCAT_WS, S, 0, b.colref(1, S), b.colref(0, S),
                    b.colref(1, S))
        return b.projection(src, [ws])
    _reject(plan, "separator", "constant")


def test_build_rejects_cast_of_decimal():
    def plan(b, src):
        d = b.call(GX_F_CAST_DEC, GX_TYPE_DECIMAL, 2, b.colref(2, I))
        return b.projection(src, [b.call(GX_F_CAST_STR, S, 0, d)])
    _reject(plan, "CAST_STR", "decimal")

    def plan_time(b, src):
        return b.projection(src, [b.call(GX_F_CAST_STR, S, 0,
                                         b.colref(3, GX_TYPE_TIME))])
    _reject(plan_time, "CAST_STR", "time")


def test_build_rejects_group_key_and_predicate():
    def agg(b, src):
        proj = b.projection(src, [mk(b, PLANS["concat_dash"])])
        return b.hashagg(proj, [b.colref(0, S)], [(GX_AGG_COUNT, -1, 0)])
    _reject(agg, "group keys")

    def pred(b, src):
        like = b.call(GX_F_LIKE, I, 0, mk(b, PLANS["concat_dash"]),
                      b.const_str("a%"))
        return b.selection(src, [like])
    _reject(pred, "predicates")


# ---------------- CPU: the host evaluator ----------------

def _host_eval(e, rows):
    """gx_debug_strcat_eval of output 0 of Projection([e]) over each bound
    chunk; returns the decoded column."""
    lib = P.declare_strcat_helpers(load_product())
    b = P.Builder(lib)
    src = b.source(TYPES)
    ex = b.build(b.projection(src, [mk(b, e)]))
    assert ex.error() == ""
    got = []
    for ch in _chunks(rows):
        n = ch.columns[0].length
        want_bytes = sum(len(ev(e, r) or b"") for r in rows) + 8
        out = PyChunk([S], max(n, 1), [0], [want_bytes])
        g = out.as_gx()
        rc = lib.gx_debug_strcat_eval(ex.ex, 0, ctypes.byref(ch.as_gx()),
                                      ctypes.byref(g.cols[0]))
        assert rc == 0, ex.error()
        assert g.cols[0].length == n
        got += [r[0] for r in out.rows(n)]
    ex.free()
    b.free()
    return got


def test_i64_text():
    vals = [0, 2 ** 63 - 1, -2 ** 63, None]
    for k in range(19):
        vals += [10 ** k, -10 ** k, 10 ** k - 1, -(10 ** k - 1)]
    rows = [(b"", b"", v, None, None) for v in vals]
    got = _host_eval(PLANS["cast_alone"], rows)
    assert got == [None if v is None else str(v) for v in vals]
    assert got[2] == "-9223372036854775808" and len(got[2]) == 20


@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("name", HOST_PLANS)
def test_host_eval_matches_model(name, n):
    rows = _rows(n)
    got = _host_eval(PLANS[name], rows)
    assert got == [dec(ev(PLANS[name], r)) for r in rows]


def test_host_eval_rejects_vm_argument():
    lib = P.declare_strcat_helpers(load_product())
    b = P.Builder(lib)
    src = b.source(TYPES)
    ex = b.build(b.projection(src, [mk(b, PLANS["concat_year_len"]),
                                    b.colref(0, S)]))
    ch = _chunks(_rows(1))[0]
    out = PyChunk([S], 1, [0], [64])
    g = out.as_gx()
    for col in (0, 1):  # a VM-computed argument; not a composed output
        rc = lib.gx_debug_strcat_eval(ex.ex, col, ctypes.byref(ch.as_gx()),
                                      ctypes.byref(g.cols[0]))
        assert rc == -1
    ex.free()
    b.free()


def test_vm_program_dump_lists_composed_programs():
    """Plans without composed outputs keep their dump (pinned by
    tests/test_vm_programs.py); a plan with one appends its own section."""
    lib = load_product()
    lib.gx_debug_vm_program.restype = ctypes.c_char_p
    lib.gx_debug_vm_program.argtypes = [ctypes.c_void_p]
    b = P.Builder(lib)
    src = b.source(TYPES)
    plain = b.build(b.projection(src, [mk(b, ("upper", S0))]))
    comp = b.build(b.projection(src, [mk(b, PLANS["ws_comma"])]))
    d0 = lib.gx_debug_vm_program(plain.ex).decode()
    d1 = lib.gx_debug_vm_program(comp.ex).decode()
    plain.free()
    comp.free()
    b.free()
    assert "strcat" not in d0
    assert "strcat[0] nPieces=3 ws=1" in d1


# ---------------- GPU ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_plans_match_model(n):
    """All eight plans in one projection (eight composed outputs, two hidden
    integer arguments) over 0..3000 rows."""
    rows = _rows(n)
    exprs = list(PLANS.values())
    got, = _project(exprs, rows, [S] * len(exprs))
    _check_cols(got, rows, exprs)


@pytest.mark.gpu
def test_nested_concat_equals_flat():
    rows = _rows(257)
    exprs = [PLANS["concat_nested"], FLAT_OF_NESTED]
    got, = _project(exprs, rows, [S, S])
    _check_cols(got, rows, exprs)
    assert [g[0] for g in got] == [g[1] for g in got]


@pytest.mark.gpu
def test_ws_null_positions():
    """Rows 0..7 carry every NULL combination of (s0, s1, i): first, middle,
    last and all arguments NULL; all-NULL gives '' and never NULL."""
    rows = _rows(256)
    got, = _project([PLANS["ws_comma"]], rows, [S])
    _check_cols(got, rows, [PLANS["ws_comma"]])
    assert got[7][0] == "" and got[0][0] == "a, , -5" and got[2][0] == "a, -5"
    assert all(g[0] is not None for g in got)


@pytest.mark.gpu
def test_column_all_null():
    rows = _rows(257, "s1_null")
    exprs = [PLANS["concat_dash"], PLANS["ws_comma"], PLANS["cast_alone"]]
    got, = _project(exprs, rows, [S] * 3)
    _check_cols(got, rows, exprs)
    assert all(g[0] is None for g in got)


@pytest.mark.gpu
def test_all_empty_output():
    """257 rows, 0 output bytes."""
    rows = _rows(257, "empty")
    e = ("concat", [S0, S1])
    got, = _project([e], rows, [S])
    assert [g[0] for g in got] == [""] * 257


@pytest.mark.gpu
def test_one_long_row():
    """One 70 000-byte row among short ones: past 65 535 and many strides of
    the block over one row."""
    rows = _rows(600, "long")
    exprs = [PLANS["concat_dash"], ("concat", [("upper", S0), ("cast", IC)])]
    got, = _project(exprs, rows, [S, S], cap=1 << 19)
    _check_cols(got, rows, exprs)
    assert len(got[300][0]) == 70_002 and len(got[300][1]) == 70_002


@pytest.mark.gpu
def test_dense_char_source():
    """l_returnflag / l_linestatus are dense char(1) columns of the
    generator's lineitem."""
    lib = load_product()
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    rf, ls = b.colref(P.L_RETFLAG, S), b.colref(P.L_LINESTATUS, S)
    cat = b.call(GX_F_CONCAT, S, 0, rf, ls, b.const_str("!"))
    ex = b.build(b.projection(src, [cat, rf, ls]))
    ex.bind_tpch(src, GX_TPCH_LINEITEM, 10_000)
    ex.open()
    got = ex.pull_all([S] * 3, [0] * 3, data_caps=[1 << 16] * 3)
    ex.close()
    ex.free()
    b.free()
    assert len(got) == 10_000
    assert all(c == r + l + "!" for c, r, l in got)
    assert len({c for c, _, _ in got}) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("pred", ["i_gt_0", "like_s0"])
def test_over_selection(pred):
    rows = _rows(3000)
    if pred == "i_gt_0":
        def sel(b):
            return b.call(GX_F_GT, I, 0, b.colref(2, I), b.const_i64(0))
        keep = [r for r in rows if r[2] is not None and r[2] > 0]
    else:
        def sel(b):
            return b.call(GX_F_LIKE, I, 0, b.colref(0, S), b.const_str("%a%"))
        keep = [r for r in rows if r[0] is not None and b"a" in r[0]]
    exprs = [PLANS["ws_comma"], PLANS["concat_windows"],
             PLANS["concat_year_len"], S0]
    got, = _project(exprs, rows, [S] * 4, sel=sel)
    assert 0 < len(keep) < len(rows)
    _check_cols(got, keep, exprs)


@pytest.mark.gpu
def test_mixed_projection():
    """Two composed outputs beside a windowed string, a computed decimal, a
    LENGTH and passthrough columns; the old outputs equal what the same plan
    gives without the composed ones."""
    rows = _rows(3000)
    win = ("upper", ("substr", S0, 2, 5))
    ln = ("length", S1)

    def run(with_composed):
        lib = load_product()
        b = P.Builder(lib)
        src = b.source(TYPES)
        d = b.call(GX_F_CAST_DEC, GX_TYPE_DECIMAL, 2, mk(b, ("length", S0)))
        ids = [mk(b, win), d, mk(b, ln), b.colref(0, S), b.colref(2, I)]
        types = [S, GX_TYPE_DECIMAL, I, S, I]
        fracs = [0, 2, 0, 0, 0]
        if with_composed:
            ids = [mk(b, PLANS["ws_comma"])] + ids + \
                  [mk(b, PLANS["concat_year_len"])]
            types = [S] + types + [S]
            fracs = [0] + fracs + [0]
        ex = b.build(b.projection(src, ids))
        ex.bind_chunks(src, _chunks(rows))
        ex.open()
        out = ex.pull_all(types, fracs,
                          data_caps=[1 << 18 if t == S else None
                                     for t in types])
        ex.close()
        ex.free()
        b.free()
        return out

    got = run(True)
    old = run(False)
    assert [g[1:6] for g in got] == old
    _check_cols([(g[0], g[1], g[3], g[4], g[5], g[6]) for g in got], rows,
                [PLANS["ws_comma"], win, ln, S0, IC,
                 PLANS["concat_year_len"]])
    want_dec = [None if r[0] is None else f"{len(r[0])}.00" for r in rows]
    assert [g[2] for g in got] == want_dec


@pytest.mark.gpu
def test_reopen():
    rows = _rows(3000)
    exprs = [PLANS["concat_windows"], PLANS["concat_year_len"],
             PLANS["ws_comma"]]
    first, second = _project(exprs, rows, [S] * 3, opens=2)
    _check_cols(first, rows, exprs)
    assert second == first
