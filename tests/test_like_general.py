"""General LIKE / NOT LIKE (GX_F_LIKE / GX_F_NOT_LIKE, include/gx_executor.h):
binary collation, byte semantics -- stringutil.CompilePatternBinary +
DoMatchBinary restated. The frozen oracle has no general LIKE, so the
reference is the Python model below (compile_pat / match), itself anchored
against an independent regex translation.

CPU: the model, the product's host-side compiler and matcher
(gx_like_compile / gx_like_match -- the same matcher source the kernels
run), and the plan-error surface.
GPU: every filter site (standalone Selection incl. OR groups, the fused
scan->filter->agg CNF interpreted and hipRTC, dense char(1) columns, join
build/probe-side predicates, the post-join other condition) and value
context (Projection, fused-aggregate VM).
"""
import ctypes
import functools
import random
import re

import numpy as np
import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_AGG_SUM, GX_F_EQ, GX_F_IF, GX_F_MUL,
                         GX_F_OR, GX_TPCH_LINEITEM, GX_TYPE_DECIMAL,
                         GX_TYPE_I64, GX_TYPE_STRING, load_oracle,
                         load_product)
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk
from tidb_amd.plan import GX_F_LIKE, GX_F_NOT_LIKE

# ---------------------------------------------------------------- model ----
M, O, A = 0, 1, 2


def compile_pat(p, esc=92):            # p: bytes
    ch, tp, last, i = [], [], False, 0
    while i < len(p):
        c = p[i]
        if c == esc:
            last, t = False, M
            if i < len(p) - 1:
                i += 1
                c = p[i]
                if not (c == esc or c == 95 or c == 37):
                    i -= 1
                    c = esc
        elif c == 95:
            if last:
                ch[-1], tp[-1] = 95, O
                ch.append(37)
                tp.append(A)
                i += 1
                continue
            t = O
        elif c == 37:
            if last:
                i += 1
                continue
            t, last = A, True
        else:
            t, last = M, False
        ch.append(c)
        tp.append(t)
        i += 1
    return ch, tp


def match(s, ch, tp):                  # recursive definition (reference)
    si = i = 0
    while i < len(ch):
        if tp[i] == M:
            if si >= len(s) or s[si] != ch[i]:
                return False
            si += 1
        elif tp[i] == O:
            if si >= len(s):
                return False
            si += 1
        else:
            i += 1
            if i == len(ch):
                return True
            while si < len(s):
                if (tp[i] == M and ch[i] == s[si]) or tp[i] == O:
                    if match(s[si:], ch[i:], tp[i:]):
                        return True
                si += 1
            return False
        i += 1
    return si == len(s)


def iter_match(s, ch, tp):             # the shape the device loop takes
    si = pi = 0
    star = -1
    ss = 0
    while si < len(s):
        if pi < len(ch) and (tp[pi] == O or (tp[pi] == M and ch[pi] == s[si])):
            si += 1
            pi += 1
        elif pi < len(ch) and tp[pi] == A:
            star = pi
            pi += 1
            ss = si
        elif star >= 0:
            pi = star + 1
            ss += 1
            si = ss
        else:
            return False
    while pi < len(ch) and tp[pi] == A:
        pi += 1
    return pi == len(ch)


def regex_match(s, ch, tp):
    """Independent translation: MATCH -> escaped byte, ONE -> ., ANY -> .*"""
    rx = b"(?s)" + b"".join(
        re.escape(bytes([c])) if t == M else (b"." if t == O else b".*")
        for c, t in zip(ch, tp))
    return re.fullmatch(rx, s) is not None


def like(s, pat, esc=92):
    """SQL value of <s LIKE pat>: None for a NULL string."""
    if s is None:
        return None
    ch, tp = compile_pat(_b(pat), esc)
    return match(_b(s), ch, tp)


def _b(x):
    return x.encode() if isinstance(x, str) else x


# ------------------------------------------------------- corpus/patterns ----
STRS = ["hello world", "", "A", "BUILDING", "mixed-Case-Str",
        "a-rather-long-string-beyond-sixteen-bytes", "trail  ", "  lead", None,
        "x", "100%", "50% off_now", "a_b", "a\\b", "\\",
        "special packages requests", "specialrequests", "requests special",
        "abababac", "aaa", "%", "_", "green forest green"]
NONNULL = [s for s in STRS if s is not None]

# (pattern, escape byte, distinct non-NULL corpus strings the model matches)
PATTERNS = [
    ("%", 92, 22), ("", 92, 1), ("_", 92, 5), ("A", 92, 1), ("a", 92, 0),
    ("BUILD%", 92, 1), ("%ING", 92, 1), ("%Case%", 92, 1),
    ("%special%requests%", 92, 2), ("h_llo%", 92, 1), ("%o w%", 92, 1),
    ("_%_", 92, 16), ("%_", 92, 21), ("%%x", 92, 1), ("%abac", 92, 1),
    ("a%a%a", 92, 1), ("%ab%ac", 92, 1), ("100\\%", 92, 1), ("%\\_%", 92, 3),
    ("a\\\\b", 92, 1), ("a\\b", 92, 1), ("trail", 92, 0), ("trail%", 92, 1),
    ("%  ", 92, 1), ("\\", 92, 1), ("%green%green%", 92, 1),
    ("50|% off|_now", 124, 1), ("%|%%", 124, 3), ("%_" * 17 + "%", 92, 3),
    ("%a-rather-long-string-beyond-si%", 92, 1),
]
PAT_IDS = [f"p{i}" for i in range(len(PATTERNS))]
PAT33 = "a" * 33   # compiles to 33 elements: one past the engine limit


def _random_pairs():
    rng = random.Random(7)
    alpha = b"ab%_\\"
    out = []
    for _ in range(20000):
        p = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 8)))
        s = bytes(rng.choice(alpha) for _ in range(rng.randint(0, 10)))
        out.append((p, s))
    return out


@functools.lru_cache(maxsize=None)
def _corpus(n=3000, seed=5):
    """Bound as <=1000-row chunks (operators emit <=1024 rows per Next);
    second column k is an i64 in 0..5."""
    rng = np.random.default_rng(seed)
    rows = []
    chunks = []
    for base in range(0, n, 1000):
        m = min(1000, n - base)
        ch = PyChunk([GX_TYPE_STRING, GX_TYPE_I64], m, [0, 0], [m * 48, None])
        for _i in range(m):
            s = STRS[rng.integers(0, len(STRS))]
            rows.append((s, int(rng.integers(0, 6))))
            ch.append_row([s, rows[-1][1]])
        chunks.append(ch)
    return chunks, rows


def _like_call(b, func, col_expr, pat, esc=92):
    args = [col_expr, b.const_str(pat)]
    if esc != 92:
        args.append(b.const_i64(esc))
    return b.call(func, GX_TYPE_I64, 0, *args)


# ------------------------------------------------------------ CPU tests ----
def test_model_counts():
    """The GPU tests compare against the model; pin what the model says."""
    for pat, esc, want in PATTERNS:
        got = sum(1 for s in NONNULL if like(s, pat, esc))
        assert got == want, (pat, got, want)
    assert len(compile_pat(b"%special%requests%")[0]) == 18
    assert len(compile_pat(_b("%_" * 17 + "%"))[0]) == 18
    assert len(compile_pat(b"%a-rather-long-string-beyond-si%")[0]) == 32
    assert len(compile_pat(_b(PAT33))[0]) == 33


def test_patterns_discriminate():
    """Every pattern but the three degenerate ones both accepts and rejects
    some non-NULL corpus string, so an always-true / always-false matcher
    cannot pass the GPU tests."""
    for pat, esc, _ in PATTERNS:
        if pat in ("%", "a", "trail"):
            continue
        hits = [bool(like(s, pat, esc)) for s in NONNULL]
        assert any(hits) and not all(hits), pat


def test_model_anchor():
    """recursive == iterative == regex translation, corpus x patterns and
    20,000 random pairs over the alphabet ab%_\\."""
    for pat, esc, _ in PATTERNS:
        ch, tp = compile_pat(_b(pat), esc)
        for s in NONNULL:
            r = match(_b(s), ch, tp)
            assert r == iter_match(_b(s), ch, tp) == regex_match(_b(s), ch, tp)
    n_match = 0
    for p, s in _random_pairs():
        ch, tp = compile_pat(p)
        r = match(s, ch, tp)
        assert r == iter_match(s, ch, tp) == regex_match(s, ch, tp), (p, s)
        n_match += r
    assert 0 < n_match < 20000


def _like_lib():
    return P.declare_like_helpers(load_product())


def _lib_compile(lib, p, esc, cap=32):
    ch = (ctypes.c_uint8 * max(cap, 1))()
    tp = (ctypes.c_uint8 * max(cap, 1))()
    n = lib.gx_like_compile(p, len(p), esc, ch, tp, cap)
    return n, list(ch[:max(n, 0)]), list(tp[:max(n, 0)])


def test_product_compile_matches_model():
    lib = _like_lib()
    cases = [(_b(p), e) for p, e, _ in PATTERNS]
    cases += [(p, 92) for p, _ in _random_pairs()]
    for p, esc in cases:
        n, ch, tp = _lib_compile(lib, p, esc)
        wch, wtp = compile_pat(p, esc)
        assert n == len(wch), p
        assert tp == wtp, p
        # MATCH elements carry their literal; ONE/ANY chars are don't-care
        assert [c for c, t in zip(ch, tp) if t == M] == \
            [c for c, t in zip(wch, wtp) if t == M], p
    assert _lib_compile(lib, _b(PAT33), 92)[0] < 0
    assert _lib_compile(lib, _b(PAT33), 92, cap=33)[0] == 33
    assert _lib_compile(lib, b"a%", 256)[0] < 0


def test_product_match_matches_model():
    lib = _like_lib()
    for pat, esc, _ in PATTERNS:
        for s in NONNULL:
            got = lib.gx_like_match(_b(pat), len(_b(pat)), esc, _b(s),
                                    len(_b(s)))
            assert got == int(like(s, pat, esc)), (pat, s)
    seen = set()
    for p, s in _random_pairs():
        ch, tp = compile_pat(p)
        want = int(match(s, ch, tp))
        assert lib.gx_like_match(p, len(p), 92, s, len(s)) == want, (p, s)
        seen.add(want)
    assert seen == {0, 1}
    assert lib.gx_like_match(_b(PAT33), 33, 92, b"a", 1) < 0


def _expect_error(build_fn, *needles):
    lib = load_product()
    b = P.Builder(lib)
    root = build_fn(b, lib)
    ex = b.build(root)
    rc = lib.gx_open(ex.ex)
    err = ex.error()
    ex.free()
    b.free()
    assert rc == -1, f"expected GX_ERR_INVALID at plan compile, got rc={rc}: {err}"
    assert all(n in err for n in needles), err


@pytest.mark.parametrize("site", ["selection", "fused", "projection"])
def test_plan_error_pattern_too_long(site):
    def plan(b, lib):
        src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
        cond = _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), PAT33)
        if site == "selection":
            return b.selection(src, [cond])
        if site == "projection":
            return b.projection(src, [cond])
        return b.hashagg(b.selection(src, [cond]), [b.colref(1, GX_TYPE_I64)],
                         [(GX_AGG_COUNT, -1, 0)])
    _expect_error(plan, "LIKE", "32")


def test_plan_error_non_constant_pattern():
    def plan(b, lib):
        src = b.source([GX_TYPE_STRING, GX_TYPE_STRING])
        cond = b.call(GX_F_LIKE, GX_TYPE_I64, 0, b.colref(0, GX_TYPE_STRING),
                      b.colref(1, GX_TYPE_STRING))
        return b.selection(src, [cond])
    _expect_error(plan, "LIKE", "constant")


def test_plan_error_non_column_argument():
    def plan(b, lib):
        src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
        cond = b.call(GX_F_NOT_LIKE, GX_TYPE_I64, 0, b.const_str("abc"),
                      b.const_str("a%"))
        return b.selection(src, [cond])
    _expect_error(plan, "LIKE", "column")


def test_plan_error_escape_out_of_range():
    def plan(b, lib):
        src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
        cond = _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), "a%", 256)
        return b.selection(src, [cond])
    _expect_error(plan, "LIKE", "escape")


def test_plan_error_value_context_in_joinagg():
    """The Q3-class join-aggregate pipeline's probe VM has no LIKE."""
    from tests.gxlib import GX_F_GT, GX_F_LT, GX_F_MINUS
    def plan(b, lib):
        cust = b.source(P.CUSTOMER_TYPES)
        sel_c = b.selection(cust, [b.call(
            GX_F_EQ, GX_TYPE_I64, 0, b.colref(P.C_MKTSEGMENT, GX_TYPE_STRING),
            b.const_str("BUILDING"))])
        orders = b.source(P.ORDERS_TYPES)
        sel_o = b.selection(orders, [b.call(
            GX_F_LT, GX_TYPE_I64, 0, b.colref(P.O_ORDERDATE, 3),
            b.const_time(lib.gx_time_from_date(1995, 3, 15)))])
        j1 = b.hashjoin(sel_c, sel_o, [b.colref(P.C_CUSTKEY, GX_TYPE_I64)],
                        [b.colref(P.O_CUSTKEY, GX_TYPE_I64)])
        li = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
        sel_l = b.selection(li, [b.call(
            GX_F_GT, GX_TYPE_I64, 0, b.colref(P.L_SHIPDATE, 3),
            b.const_time(lib.gx_time_from_date(1995, 3, 15)))])
        j2 = b.hashjoin(j1, sel_l, [b.colref(2, GX_TYPE_I64)],
                        [b.colref(P.L_ORDERKEY, GX_TYPE_I64)])
        price = b.colref(6 + P.L_EXTPRICE, GX_TYPE_DECIMAL, 2)
        flag = _like_call(b, GX_F_LIKE,
                          b.colref(6 + P.L_RETFLAG, GX_TYPE_STRING), "%A%")
        val = b.call(GX_F_MUL, GX_TYPE_DECIMAL, 2, price, flag)
        proj = b.projection(j2, [b.colref(6 + P.L_ORDERKEY, GX_TYPE_I64),
                                 b.colref(4, 3), b.colref(5, GX_TYPE_I64),
                                 val])
        agg = b.hashagg(proj, [b.colref(0, GX_TYPE_I64), b.colref(1, 3),
                               b.colref(2, GX_TYPE_I64)],
                        [(GX_AGG_SUM, b.colref(3, GX_TYPE_DECIMAL, 2), 2)])
        return b.topn(agg, [b.colref(3, GX_TYPE_DECIMAL, 2), b.colref(1, 3)],
                      [1, 0], 10)
    _expect_error(plan, "LIKE", "join-aggregate")


# ------------------------------------------------------------ GPU tests ----
def _pull(b, root, binds, types, caps):
    ex = b.build(root)
    for src, chunks in binds:
        ex.bind_chunks(src, chunks)
    ex.open()
    out = ex.pull_all(types, [0] * len(types), data_caps=caps)
    ex.close()
    ex.free()
    b.free()
    return out


def _run_selection(conds_fn):
    chunks, rows = _corpus()
    b = P.Builder(load_product())
    src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
    root = b.selection(src, conds_fn(b))
    out = _pull(b, root, [(src, chunks)], [GX_TYPE_STRING, GX_TYPE_I64],
                [1 << 18, None])
    return out, rows


@pytest.mark.gpu
@pytest.mark.parametrize("pat,esc,_n", PATTERNS, ids=PAT_IDS)
def test_selection_like(pat, esc, _n):
    got, rows = _run_selection(lambda b: [_like_call(
        b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), pat, esc)])
    assert got == [(s, k) for s, k in rows if like(s, pat, esc)]


@pytest.mark.gpu
@pytest.mark.parametrize("pat", ["%ING", "%abac", "_%_", "%"])
def test_selection_not_like(pat):
    got, rows = _run_selection(lambda b: [_like_call(
        b, GX_F_NOT_LIKE, b.colref(0, GX_TYPE_STRING), pat)])
    assert got == [(s, k) for s, k in rows if like(s, pat) is False]
    assert all(s is not None for s, _ in got)


@pytest.mark.gpu
def test_selection_or_group_and_not_like():
    """(s LIKE '%ING' OR k = 3) AND s NOT LIKE 'h%': a NULL LIKE leaf is
    false inside the OR group and rejects the row as a conjunct."""
    def conds(b):
        s = b.colref(0, GX_TYPE_STRING)
        grp = b.call(GX_F_OR, GX_TYPE_I64, 0,
                     _like_call(b, GX_F_LIKE, s, "%ING"),
                     b.call(GX_F_EQ, GX_TYPE_I64, 0, b.colref(1, GX_TYPE_I64),
                            b.const_i64(3)))
        return [grp, _like_call(b, GX_F_NOT_LIKE, s, "h%")]
    got, rows = _run_selection(conds)
    want = [(s, k) for s, k in rows
            if (like(s, "%ING") or k == 3) and like(s, "h%") is False]
    assert got == want and len(want) > 0
    assert any(k != 3 for _, k in want) and any(k == 3 for _, k in want)


@pytest.mark.gpu
def test_selection_two_patterns():
    got, rows = _run_selection(lambda b: [
        _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), "%special%"),
        _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), "%requests")])
    want = [(s, k) for s, k in rows
            if like(s, "%special%") and like(s, "%requests")]
    assert got == want and len(want) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("no_jit", [False, True], ids=["hiprtc", "interp"])
@pytest.mark.parametrize("pat", ["%special%requests%", "%abac", "_%_"])
def test_fused_agg_like(pat, no_jit, monkeypatch):
    """WHERE s LIKE p GROUP BY s, count(*) over bound chunks. String group
    keys are PAD SPACE: the device emits the group value with its trailing
    spaces trimmed (tests/test_wide_groupkeys.py), so the model groups on
    the trimmed value -- no two corpus strings collide under that."""
    if no_jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    else:
        monkeypatch.delenv("GX_NO_JIT", raising=False)
    chunks, rows = _corpus()
    b = P.Builder(load_product())
    src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
    sel = b.selection(src, [_like_call(b, GX_F_LIKE,
                                       b.colref(0, GX_TYPE_STRING), pat)])
    agg = b.hashagg(sel, [b.colref(0, GX_TYPE_STRING)],
                    [(GX_AGG_COUNT, -1, 0)])
    got = _pull(b, agg, [(src, chunks)], [GX_TYPE_STRING, GX_TYPE_I64],
                [1 << 16, None])
    want = {}
    for s, _k in rows:
        if like(s, pat):
            want[s.rstrip(" ")] = want.get(s.rstrip(" "), 0) + 1
    assert sorted(got) == sorted(want.items()) and len(want) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("no_jit", [False, True], ids=["hiprtc", "interp"])
def test_fused_agg_like_packed_key(no_jit, monkeypatch):
    """Same filter with an i64 group key: the packed-key shape is the one the
    hipRTC specialization takes (string keys run the interpreted kernel)."""
    if no_jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    else:
        monkeypatch.delenv("GX_NO_JIT", raising=False)
    chunks, rows = _corpus()
    b = P.Builder(load_product())
    src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
    sel = b.selection(src, [
        _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), "%a%a%"),
        _like_call(b, GX_F_NOT_LIKE, b.colref(0, GX_TYPE_STRING), "%c")])
    agg = b.hashagg(sel, [b.colref(1, GX_TYPE_I64)], [(GX_AGG_COUNT, -1, 0)])
    got = _pull(b, agg, [(src, chunks)], [GX_TYPE_I64, GX_TYPE_I64],
                [None, None])
    want = {}
    for s, k in rows:
        if like(s, "%a%a%") and like(s, "%c") is False:
            want[k] = want.get(k, 0) + 1
    assert sorted(got) == sorted(want.items()) and len(want) == 6


def _run_lineitem(lib, cond_fn):
    """The group-by of tests/test_string_builtins._run_fused_string_filter."""
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    rf = b.colref(P.L_RETFLAG, GX_TYPE_STRING)
    cond = cond_fn(b, rf)
    child = b.selection(src, [cond]) if cond is not None else src
    qty = b.colref(P.L_QUANTITY, GX_TYPE_DECIMAL, 2)
    ls = b.colref(P.L_LINESTATUS, GX_TYPE_STRING)
    agg = b.hashagg(child, [ls], [(GX_AGG_SUM, qty, 2), (GX_AGG_COUNT, -1, 0)])
    ex = b.build(agg)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, 100_000)
    ex.open()
    rows = ex.pull_all([GX_TYPE_STRING, GX_TYPE_DECIMAL, GX_TYPE_I64],
                       [0, 2, 0], data_caps=[2048, None, None])
    ex.close()
    ex.free()
    b.free()
    return sorted(rows)


@pytest.mark.gpu
def test_dense_char_column_vs_oracle():
    """Dense char(1) column (denseOffsets), anchored on the ORACLE: LIKE
    '%A%' over one byte is = 'A'; LIKE '_' keeps every row."""
    want_a = _run_lineitem(load_oracle(), lambda b, rf: b.call(
        GX_F_EQ, GX_TYPE_I64, 0, rf, b.const_str("A")))
    got_a = _run_lineitem(load_product(), lambda b, rf: _like_call(
        b, GX_F_LIKE, rf, "%A%"))
    assert got_a == want_a and len(got_a) == 2
    want_all = _run_lineitem(load_oracle(), lambda b, rf: None)
    got_all = _run_lineitem(load_product(), lambda b, rf: _like_call(
        b, GX_F_LIKE, rf, "_"))
    assert got_all == want_all
    assert sum(r[2] for r in got_all) == 100_000


def _join_sides():
    rng = np.random.default_rng(17)

    def side(n):
        rows = [(int(rng.integers(0, 10)), STRS[rng.integers(0, len(STRS))])
                for _ in range(n)]
        ch = PyChunk([GX_TYPE_I64, GX_TYPE_STRING], n, [0, 0], [None, n * 48])
        for r in rows:
            ch.append_row(list(r))
        return rows, [ch]
    return side(40), side(300)


JOIN_TYPES = [GX_TYPE_I64, GX_TYPE_STRING, GX_TYPE_I64, GX_TYPE_STRING]


@pytest.mark.gpu
def test_join_side_predicates():
    """LIKE on the build side, NOT LIKE on the probe side of a hash join."""
    (brows, bch), (prows, pch) = _join_sides()
    b = P.Builder(load_product())
    bsrc = b.source([GX_TYPE_I64, GX_TYPE_STRING])
    psrc = b.source([GX_TYPE_I64, GX_TYPE_STRING])
    bsel = b.selection(bsrc, [_like_call(
        b, GX_F_LIKE, b.colref(1, GX_TYPE_STRING), "%a%")])
    psel = b.selection(psrc, [_like_call(
        b, GX_F_NOT_LIKE, b.colref(1, GX_TYPE_STRING), "%special%")])
    j = b.hashjoin(bsel, psel, [b.colref(0, GX_TYPE_I64)],
                   [b.colref(0, GX_TYPE_I64)])
    got = _pull(b, j, [(bsrc, bch), (psrc, pch)], JOIN_TYPES,
                [None, 1 << 20, None, 1 << 20])
    want = [(bk, bs, pk, ps) for bk, bs in brows if like(bs, "%a%")
            for pk, ps in prows
            if like(ps, "%special%") is False and bk == pk]
    assert sorted(got) == sorted(want) and len(want) > 0


@pytest.mark.gpu
def test_join_other_condition_like():
    """LIKE leaves in the post-join other condition, alone and in an OR
    group, on a build-side and a probe-side output column."""
    (brows, bch), (prows, pch) = _join_sides()
    b = P.Builder(load_product())
    bsrc = b.source([GX_TYPE_I64, GX_TYPE_STRING])
    psrc = b.source([GX_TYPE_I64, GX_TYPE_STRING])
    j = b.hashjoin(bsrc, psrc, [b.colref(0, GX_TYPE_I64)],
                   [b.colref(0, GX_TYPE_I64)])
    grp = b.call(GX_F_OR, GX_TYPE_I64, 0,
                 _like_call(b, GX_F_LIKE, b.colref(1, GX_TYPE_STRING), "%ab%ac"),
                 _like_call(b, GX_F_LIKE, b.colref(1, GX_TYPE_STRING), "_"))
    root = b.selection(j, [grp, _like_call(
        b, GX_F_LIKE, b.colref(3, GX_TYPE_STRING), "%e%")])
    got = _pull(b, root, [(bsrc, bch), (psrc, pch)], JOIN_TYPES,
                [None, 1 << 20, None, 1 << 20])
    want = [(bk, bs, pk, ps) for bk, bs in brows for pk, ps in prows
            if bk == pk and (like(bs, "%ab%ac") or like(bs, "_"))
            and like(ps, "%e%")]
    assert sorted(got) == sorted(want) and len(want) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("pat", ["%a%", "_%_", "%special%requests%"])
def test_projection_value_context(pat):
    """[s LIKE p, s NOT LIKE p, IF(s LIKE p, k, -1)]: NULL strings give
    NULL, NULL and the else branch."""
    chunks, rows = _corpus()
    b = P.Builder(load_product())
    src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
    s = b.colref(0, GX_TYPE_STRING)
    lk = _like_call(b, GX_F_LIKE, s, pat)
    root = b.projection(src, [
        lk, _like_call(b, GX_F_NOT_LIKE, s, pat),
        b.call(GX_F_IF, GX_TYPE_I64, 0, lk, b.colref(1, GX_TYPE_I64),
               b.const_i64(-1))])
    got = _pull(b, root, [(src, chunks)], [GX_TYPE_I64] * 3, [None] * 3)

    def i(v):
        return None if v is None else int(v)
    want = [(i(like(s_, pat)), i(None if s_ is None else not like(s_, pat)),
             k if like(s_, pat) else -1) for s_, k in rows]
    assert got == want
    assert any(w[0] is None for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("no_jit", [False, True], ids=["hiprtc", "interp"])
def test_fused_value_context(no_jit, monkeypatch):
    """sum(CAST_DEC(IF(s LIKE '%a%', k, 0))) GROUP BY k."""
    if no_jit:
        monkeypatch.setenv("GX_NO_JIT", "1")
    else:
        monkeypatch.delenv("GX_NO_JIT", raising=False)
    chunks, rows = _corpus()
    b = P.Builder(load_product())
    src = b.source([GX_TYPE_STRING, GX_TYPE_I64])
    k = b.colref(1, GX_TYPE_I64)
    iff = b.call(GX_F_IF, GX_TYPE_I64, 0,
                 _like_call(b, GX_F_LIKE, b.colref(0, GX_TYPE_STRING), "%a%"),
                 k, b.const_i64(0))
    dec = b.call(20, GX_TYPE_DECIMAL, 0, iff)  # GX_F_CAST_DEC
    agg = b.hashagg(src, [k], [(GX_AGG_SUM, dec, 0), (GX_AGG_COUNT, -1, 0)])
    got = _pull(b, agg, [(src, chunks)],
                [GX_TYPE_I64, GX_TYPE_DECIMAL, GX_TYPE_I64], [None] * 3)
    want = {}
    for s, kk in rows:
        t, c = want.get(kk, (0, 0))
        want[kk] = (t + (kk if like(s, "%a%") else 0), c + 1)
    assert sorted(got) == sorted((kk, str(t), c)
                                 for kk, (t, c) in want.items())
    assert any(t > 0 for t, _ in want.values())
