"""Every VM opcode at every site that executes it, against the oracle.

The expression VM (VmIns, gx_common.h) runs in four interpreting kernels
(fused aggregate, its glds-staged variant, the join-aggregate probe and
Projection) and in two hipRTC generators. One 300-row table -- more than one
256-thread block with a partial tail, and above the staged kernel's 256-row
floor -- carries three decimal columns of different frac, an int64, a
datetime and a string column with ~10% NULLs each, zero divisors, and a
6-row tail whose products overflow the int64 VM so the int128 retry runs.
The first 294 rows never overflow: runs over them are answered by the
narrow kernels, runs over all 300 by the wide ones.

The same expression groups run through Projection (narrow; wide, next to
an overflowing a * b), and as
sum(expr) GROUP BY g through the generated kernel, the interpreter
(GX_NO_JIT) and the forced int128 VM (GX_FORCE_WIDE). Comparison with the
oracle is exact (decimals by value, NULL as NULL).

Two things the sites themselves rule out:
  * Projection's opcode set on the host (kVmOpsProject, gx_engine.cpp) is
    the full set without VM_DIV, so `/` runs in the aggregate cases only.
  * The oracle has no general LIKE. Its plan spells the same pattern,
    'ab%', with GX_F_LIKE_PREFIX; the product plan uses GX_F_LIKE, which is
    what lowers to VM_LIKE.
ABS stays away from INT64_MIN: the oracle's own handling of it is undefined.
"""
import ctypes
import functools
from decimal import Decimal

import numpy as np
import pytest

from tests.gxlib import (GX_AGG_SUM, GX_F_ABS, GX_F_CAST_DEC, GX_F_CAST_INT,
                         GX_F_DAY, GX_F_DIV, GX_F_GREATEST, GX_F_GT, GX_F_HOUR,
                         GX_F_IF, GX_F_IFNULL, GX_F_LE, GX_F_LEAST,
                         GX_F_LENGTH, GX_F_LIKE_PREFIX, GX_F_MINUS,
                         GX_F_MINUTE, GX_F_MONTH, GX_F_MUL, GX_F_PLUS,
                         GX_F_ROUND, GX_F_SECOND, GX_F_YEAR, GX_TYPE_DECIMAL,
                         GX_TYPE_I64, GX_TYPE_STRING, GX_TYPE_TIME,
                         load_oracle, load_product)
from tidb_amd import plan as P
from tidb_amd.chunkpy import PyChunk
from tidb_amd.plan import GX_F_LIKE

# columns: group key, decimals of frac 2 / 4 / 0, int64, datetime, string
G, A, B, C, K, T, S = range(7)
TYPES = [GX_TYPE_I64, GX_TYPE_DECIMAL, GX_TYPE_DECIMAL, GX_TYPE_DECIMAL,
         GX_TYPE_I64, GX_TYPE_TIME, GX_TYPE_STRING]
FRACS = [0, 2, 4, 0, 0, 0, 0]
N_ROWS = 300
N_PLAIN = 294  # rows before the overflow tail
WORDS = ["", "a", "ab", "abc", "abacus", "ab%", "b", "ba", "zab", "absolutely",
         "Ab", "a b", "abababababab"]


@functools.lru_cache(maxsize=None)
def _rows(nulls):
    """(g, a, b, c, k, (y,m,d,h,mi,s), s) with decimals as strings."""
    rng = np.random.default_rng(20261)

    def maybe(v):
        return None if nulls and rng.random() < 0.1 else v

    def dec(int_hi, frac):
        sign = "-" if rng.random() < 0.5 else ""
        s = f"{sign}{int(rng.integers(0, int_hi))}"
        if frac:
            s += f".{int(rng.integers(0, 10 ** frac)):0{frac}d}"
        return s

    rows = []
    for i in range(N_ROWS):
        big = i >= N_PLAIN
        g = int(rng.integers(0, 5))
        if big:  # |a * b| ~ 9e35 units: past int64, inside int128
            sign = "-" if i % 2 else ""
            a = f"{sign}9{int(rng.integers(0, 10 ** 15)):015d}.37"
            b = f"9{int(rng.integers(0, 10 ** 13)):013d}.9999"
        else:
            a = maybe(dec(100000, 2))
            b = maybe(dec(1000, 4))
        # about one divisor in six is zero
        c = maybe("0" if rng.random() < 0.17 else dec(50, 0))
        k = maybe(int(rng.integers(-1000, 1001)))
        t = maybe((int(rng.integers(1992, 1999)), int(rng.integers(1, 13)),
                   int(rng.integers(1, 29)), int(rng.integers(0, 24)),
                   int(rng.integers(0, 60)), int(rng.integers(0, 60))))
        s = maybe(WORDS[int(rng.integers(0, len(WORDS)))])
        rows.append((g, a, b, c, k, t, s))
    return rows


def _chunk(lib, rows):
    def dec(s):
        out = (ctypes.c_uint8 * 40)()
        assert lib.gx_dec_from_string(s.encode(), len(s.encode()), out) == 0
        return bytes(out)

    ch = PyChunk(TYPES, len(rows), FRACS, [None] * 6 + [len(rows) * 16])
    for g, a, b, c, k, t, s in rows:
        ch.append_row([g] + [None if v is None else dec(v) for v in (a, b, c)]
                      + [k, None if t is None
                         else lib.gx_time_from_datetime(*t, 0, 0), s])
    return ch


TABLES = {  # name -> (nullable, row count)
    "plain": (True, N_PLAIN),
    "full": (True, N_ROWS),
    "nonull": (False, N_PLAIN),
}

# ---- expression groups: name -> fn(b, is_oracle) -> [(expr, type, frac)] ----
DEC, I64 = GX_TYPE_DECIMAL, GX_TYPE_I64


def _cols(b):
    return (b.colref(A, DEC, 2), b.colref(B, DEC, 4), b.colref(C, DEC, 0),
            b.colref(K, I64), b.colref(T, GX_TYPE_TIME),
            b.colref(S, GX_TYPE_STRING))


def _arith(b, _):
    a, bb, *_r = _cols(b)
    return [(b.call(GX_F_PLUS, DEC, 4, a, bb), DEC, 4),
            (b.call(GX_F_MINUS, DEC, 4, a, bb), DEC, 4),
            (b.call(GX_F_MUL, DEC, 6, a, bb), DEC, 6)]


def _div(b, _):
    a, _bb, c, *_r = _cols(b)
    # frac 2 / frac 0 -> word-granular result frac 9
    return [(b.call(GX_F_DIV, DEC, 9, a, c), DEC, 9)]


def _round(b, _):
    a, bb, _c, k, *_r = _cols(b)
    prod = b.call(GX_F_MUL, DEC, 6, a, bb)
    return [(b.call(GX_F_ROUND, DEC, 2, prod, b.const_i64(2)), DEC, 2),
            (b.call(GX_F_CAST_DEC, DEC, 1, bb), DEC, 1),
            (b.call(GX_F_CAST_INT, I64, 0, a), I64, 0),
            (b.call(GX_F_CAST_DEC, DEC, 1, k), DEC, 1)]


def _abs(b, _):
    a, bb, _c, k, *_r = _cols(b)
    return [(b.call(GX_F_ABS, DEC, 2, a), DEC, 2),
            (b.call(GX_F_ABS, I64, 0, k), I64, 0),
            (b.call(GX_F_IFNULL, DEC, 4, a, bb), DEC, 4)]


def _if(b, _):
    a, bb, *_r = _cols(b)
    gt = b.call(GX_F_GT, I64, 0, a, bb)
    return [(b.call(GX_F_IF, DEC, 4, gt, a, bb), DEC, 4)]


def _minmax(b, _):
    a, bb, *_r = _cols(b)
    return [(b.call(GX_F_GREATEST, DEC, 4, a, bb), DEC, 4),
            (b.call(GX_F_LEAST, DEC, 4, a, bb), DEC, 4),
            (b.call(GX_F_LE, I64, 0, a, bb), I64, 0)]


def _ymd(b, _):
    t = _cols(b)[4]
    return [(b.call(f, I64, 0, t), I64, 0)
            for f in (GX_F_YEAR, GX_F_MONTH, GX_F_DAY)]


def _hms(b, _):
    t = _cols(b)[4]
    return [(b.call(f, I64, 0, t), I64, 0)
            for f in (GX_F_HOUR, GX_F_MINUTE, GX_F_SECOND)]


def _length(b, _):
    a, s = _cols(b)[0], _cols(b)[5]
    length = b.call(GX_F_LENGTH, I64, 0, s)
    # LENGTH feeds decimal arithmetic too (int -> frac-2 alignment)
    return [(length, I64, 0), (b.call(GX_F_PLUS, DEC, 2, a, length), DEC, 2)]


def _like(b, is_oracle):
    # its own group: the generator declines plans that hold a LENGTH
    k, s = _cols(b)[3], _cols(b)[5]
    if is_oracle:
        like = b.call(GX_F_LIKE_PREFIX, I64, 0, s, b.const_str("ab"))
    else:
        like = b.call(GX_F_LIKE, I64, 0, s, b.const_str("ab%"))
    return [(like, I64, 0),
            (b.call(GX_F_IF, I64, 0, like, k, b.const_i64(-7)), I64, 0)]


GROUPS = {"arith": _arith, "div": _div, "round": _round, "abs": _abs,
          "if": _if, "minmax": _minmax, "ymd": _ymd, "hms": _hms, "length": _length,
          "like": _like}
CORE_GROUPS = ["arith", "abs", "if", "minmax", "ymd"]  # kVmOpsCore only
OVERFLOWING = ("arith", "round")  # groups that multiply a * b


def _norm(rows):
    return [tuple(Decimal(v) if isinstance(v, str) else v for v in r)
            for r in rows]


def _run(lib, is_oracle, group, kind, table):
    """kind 'proj': one output row per input row; 'projw' projects a * b
    as well (the OVERFLOWING groups hold it already), whose tail rows
    overflow int64, so the whole plan reruns on the
    int128 VM. kind 'agg': sum(expr) GROUP BY g, sorted by g (int-valued
    expressions sum as decimal(0))."""
    nulls, n = TABLES[table]
    b = P.Builder(lib)
    src = b.source(TYPES, FRACS)
    exprs = GROUPS[group](b, is_oracle)
    if kind == "projw" and group not in OVERFLOWING:
        a, bb, *_r = _cols(b)
        exprs = exprs + [(b.call(GX_F_MUL, DEC, 6, a, bb), DEC, 6)]
    if kind != "agg":
        root = b.projection(src, [e for e, _, _ in exprs])
        types = [t for _, t, _ in exprs]
        fracs = [f for _, _, f in exprs]
    else:
        aggs = [(GX_AGG_SUM,
                 e if t == DEC else b.call(GX_F_CAST_DEC, DEC, 0, e), f)
                for e, t, f in exprs]
        root = b.hashagg(src, [b.colref(G, I64)], aggs)
        types = [I64] + [DEC] * len(exprs)
        fracs = [0] + [f for _, _, f in exprs]
    ex = b.build(root)
    ex.bind_chunks(src, [_chunk(lib, _rows(nulls)[:n])])
    ex.open()
    out = ex.pull_all(types, fracs)
    ex.close()
    ex.free()
    b.free()
    out = _norm(out)
    return sorted(out) if kind == "agg" else out


@functools.lru_cache(maxsize=None)
def _want(group, kind, table):
    return _run(load_oracle(), True, group, kind, table)


def _setenv(monkeypatch, **on):
    monkeypatch.setenv("GX_DEBUG", "1")  # the engine names its path on stderr
    for var in ("GX_NO_JIT", "GX_FORCE_WIDE", "GX_GLDS"):
        if on.get(var):
            monkeypatch.setenv(var, "1")
        else:
            monkeypatch.delenv(var, raising=False)


def _check(capfd, group, kind, table):
    """Compare with the oracle; returns the engine's GX_DEBUG lines, from
    which the callers assert which kernel answered."""
    want = _want(group, kind, table)
    capfd.readouterr()
    got = _run(load_product(), False, group, kind, table)
    log = capfd.readouterr().err
    assert len(got) == len(want) == (5 if kind == "agg" else TABLES[table][1])
    assert got == want
    return log


JIT_OK = "[gx] jit ok"
WIDE_RETRY = "narrow overflow -> wide retry"


def test_table_shape():
    """The table holds what the cases below rely on."""
    rows = _rows(True)
    assert len(rows) == N_ROWS > 256
    for col in (A, B, C, K, T, S):
        n_null = sum(r[col] is None for r in rows)
        assert 15 <= n_null <= 45, (col, n_null)
    assert sum(r[C] == "0" for r in rows) >= 20
    for r in rows[N_PLAIN:]:  # the tail overflows int64, not int128
        units = abs(int(Decimal(r[A]) * 100) * int(Decimal(r[B]) * 10000))
        assert 2 ** 63 < units < 2 ** 126
    for r in rows[:N_PLAIN]:
        if r[A] is not None and r[B] is not None:
            assert abs(Decimal(r[A]) * Decimal(r[B])) * 10 ** 6 < 2 ** 62
    assert all(r[K] is None or abs(r[K]) <= 1000 for r in rows)
    assert not any(None in r for r in _rows(False)[:N_PLAIN])


PROJ_GROUPS = [g for g in GROUPS if g != "div"]


@pytest.mark.gpu
@pytest.mark.parametrize("group", PROJ_GROUPS)
def test_projection_narrow(group, monkeypatch, capfd):
    """(a) projectKernel<false>: no row overflows, the int64 VM answers."""
    _setenv(monkeypatch)
    _check(capfd, group, "proj", "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("group", PROJ_GROUPS)
def test_projection_wide(group, monkeypatch, capfd):
    """(b) projectKernel<true>. Projection reaches its int128 VM through
    the overflow retry only (it does not read GX_FORCE_WIDE, set here all
    the same), so every group is projected next to a * b: the tail rows
    overflow the narrow pass and the wide kernel evaluates the whole plan."""
    _setenv(monkeypatch, GX_FORCE_WIDE=1)
    _check(capfd, group, "projw", "full")


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["plain", "full"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_fused_generated(group, table, monkeypatch, capfd):
    """(c) the hipRTC kernel; on the full table its narrow pass overflows
    and the wide entry point reruns. The generator declines LENGTH plans,
    and says so; every other group must run generated code."""
    _setenv(monkeypatch)
    log = _check(capfd, group, "agg", table)
    if group == "length":
        assert "jit DISABLED: string builtin not specialized" in log
    else:
        assert JIT_OK in log
    if table == "full" and group in OVERFLOWING:
        assert WIDE_RETRY in log


@pytest.mark.gpu
@pytest.mark.parametrize("table", ["plain", "full"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_fused_interpreted(group, table, monkeypatch, capfd):
    """(d) GX_NO_JIT=1: processRow, narrow and (full table) wide retry."""
    _setenv(monkeypatch, GX_NO_JIT=1)
    log = _check(capfd, group, "agg", table)
    assert "[gx] jit" not in log and "useGlds=0" in log
    if table == "full" and group in OVERFLOWING:
        assert WIDE_RETRY in log


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_fused_force_wide(group, monkeypatch, capfd):
    """(e) GX_FORCE_WIDE=1: the int128 VM on values that fit int64."""
    _setenv(monkeypatch, GX_FORCE_WIDE=1)
    log = _check(capfd, group, "agg", "plain")
    assert WIDE_RETRY not in log  # wide from the start


@pytest.mark.gpu
@pytest.mark.parametrize("group", CORE_GROUPS)
def test_staged_core(group, monkeypatch, capfd):
    """GX_GLDS=1 GX_NO_JIT=1 on the NULL-free table: the glds-staged kernel
    (sum-only plans, core opcodes, 294 >= 256 rows)."""
    _setenv(monkeypatch, GX_GLDS=1, GX_NO_JIT=1)
    assert "useGlds=1" in _check(capfd, group, "agg", "nonull")


@pytest.mark.gpu
def test_staged_declines_round(monkeypatch, capfd):
    """A ROUND/CAST plan under GX_GLDS=1 is outside the staged kernel's
    opcode set and must still match the oracle, through the plain kernel.
    (The one case here that an engine whose staged eligibility test does
    not screen opcodes may fail: its staged VM skips VM_ROUND_SCALE.)"""
    _setenv(monkeypatch, GX_GLDS=1, GX_NO_JIT=1)
    assert "useGlds=0" in _check(capfd, "round", "agg", "nonull")


@pytest.mark.gpu
def test_q3_interpreted_probe(monkeypatch):
    """Q3 with GX_NO_JIT=1: the interpreted join-aggregate probe VM
    (jaProbeKernel) against the oracle."""
    from tests.test_oracle_q3 import run_q3
    _setenv(monkeypatch, GX_NO_JIT=1)
    got = run_q3(load_product())
    want = run_q3(load_oracle())
    assert len(got) == len(want) > 0
    assert got == want


@pytest.mark.gpu
def test_q3_round_leaves_the_probe(monkeypatch, capfd):
    """Q3 summing ROUND(price * (1 - disc), 2): VM_ROUND_SCALE is outside the
    probe kernel's opcode set, so the host refuses the join-aggregate
    pipeline and the plan runs as aggregation over joined rows. The TopN
    limit exceeds the group count and rows compare sorted: two-digit
    revenues tie."""
    from tests.test_oracle_q3 import run_q3
    _setenv(monkeypatch)
    want = sorted(run_q3(load_oracle(), 100000, P.round_revenue))
    capfd.readouterr()
    got = sorted(run_q3(load_product(), 100000, P.round_revenue))
    log = capfd.readouterr().err
    assert len(want) > 50
    assert got == want
    assert "[gx] ja " not in log  # no join-aggregate build or probe ran


@pytest.mark.gpu
@pytest.mark.parametrize("no_jit", [0, 1])
def test_q3_if_value_on_the_probe(no_jit, monkeypatch, capfd):
    """Q3 summing IF(disc > 0.05, price * (1 - disc), price): VM_CMP and
    VM_IF keep their third operand in ins.c, which the probe's host site
    must hand to the kernel as compiled. Generated and interpreted probe."""
    from tests.test_oracle_q3 import run_q3
    _setenv(monkeypatch, GX_NO_JIT=no_jit)
    want = sorted(run_q3(load_oracle(), 100000, P.if_revenue))
    capfd.readouterr()
    got = sorted(run_q3(load_product(), 100000, P.if_revenue))
    log = capfd.readouterr().err
    assert len(want) > 50
    assert got == want
    # differs from plain Q3: the IF took effect
    assert want != sorted(run_q3(load_oracle(), 100000))
    if not no_jit:
        assert "[gx] ja jit ok" in log
