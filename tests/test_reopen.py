"""Open/Next/Close repeated on one executor gives the same rows every time.

That is the drop-in boundary's contract and what the benchmark times. Each
case runs three open/pull/close cycles on one product executor, with a
fourth cycle after the first that is closed after a single chunk, so the
next open meets a half-drained run (test_null_slots.pull_cycles). Every
full cycle must equal the oracle's single open: row for row where the plan
orders, as a sorted multiset otherwise. Every ordering or limiting case runs
with OFFSET > 0, with and without a LIMIT: a re-open that restarts at row 0
of the kept table returns rows [0, o + l) instead of [o, o + l).

The lineitem sort keys (ship date asc, order key desc) tie on a few rows,
and the order within a tie is free: there the key columns compare row for
row and the full rows as a multiset (no tie straddles a slice boundary,
test_oracle_sort_slices).

Sites: the device sort and TopN over a generator source, over bound chunks,
and spilled to host runs (run count asserted from the log); keyless
LIMIT/OFFSET over a bare source and over a Selection; a sort above a
Selection and above an in-memory join; standalone Selection and Projection;
offsets past the input. The spilled join's re-open is in
test_join_spill_matrix.py.
"""
import functools
import re

import pytest

from tests.gxlib import (GX_F_LT, GX_TPCH_LINEITEM, load_oracle,
                         load_product)
from tests.test_full_sort import KEYS_2
from tests.test_null_slots import (I64, Scn, _check_product, _join_sort_scn,
                                   _proj_scn, _sel_scn, _sel_sort_scn, _want,
                                   pull_cycles)
from tidb_amd import plan as P

N_SORT = 8000
SORT_DESC = [0, 1]
# (limit, offset): TopN, Sort with an offset, an offset past the input
SLICES = [(100, 7), (-1, 7), (100, N_SORT + 1000)]
LI_CAPS = [None] * 5 + [2048, 2048] + [None]
SORT_KEY = lambda r: (r[P.L_SHIPDATE], r[P.L_ORDERKEY])
SPILL_SORT_RE = re.compile(r"\[gx\] spill sort: (\d+) runs")


def _gen_sort(lib, limit, offset, opens):
    b = P.Builder(lib)
    src = b.source(P.LINEITEM_TYPES, P.LINEITEM_FRACS)
    root = b.topn(src, [b.colref(c, t, f) for c, t, f in KEYS_2], SORT_DESC,
                  limit, offset)
    ex = b.build(root)
    ex.bind_tpch(src, GX_TPCH_LINEITEM, N_SORT)
    cycles = pull_cycles(ex, P.LINEITEM_TYPES, P.LINEITEM_FRACS, LI_CAPS,
                         opens)
    ex.free()
    b.free()
    return cycles


@functools.lru_cache(maxsize=None)
def _want_sort(limit, offset):
    return _gen_sort(load_oracle(), limit, offset, 1)[0]


def _assert_sorted_same(got, want):
    assert [SORT_KEY(r) for r in got] == [SORT_KEY(r) for r in want]
    assert sorted(got) == sorted(want)


def test_oracle_sort_slices():
    full = _want_sort(-1, 0)
    assert len(full) == N_SORT
    keys = [SORT_KEY(r) for r in full]
    assert keys[6] != keys[7] and keys[106] != keys[107]
    assert _want_sort(100, 7) == full[7:107]
    assert _want_sort(-1, 7) == full[7:]
    assert _want_sort(100, N_SORT + 1000) == []


@pytest.mark.gpu
@pytest.mark.parametrize("limit,offset", SLICES)
def test_reopen_sort_generator(limit, offset, monkeypatch):
    monkeypatch.delenv("GX_SORT_RUN_ROWS", raising=False)
    for rows in _gen_sort(load_product(), limit, offset, 3):
        _assert_sorted_same(rows, _want_sort(limit, offset))


@pytest.mark.gpu
@pytest.mark.parametrize("limit,offset", SLICES)
def test_reopen_sort_spilled(limit, offset, monkeypatch, capfd):
    """1500-row runs: six device-sorted runs on the host, merged again from
    the top at every open; sorted once."""
    monkeypatch.setenv("GX_DEBUG", "1")
    monkeypatch.setenv("GX_SORT_RUN_ROWS", "1500")
    capfd.readouterr()
    cycles = _gen_sort(load_product(), limit, offset, 3)
    assert SPILL_SORT_RE.findall(capfd.readouterr().err) == ["6"]
    for rows in cycles:
        _assert_sorted_same(rows, _want_sort(limit, offset))


@functools.lru_cache(maxsize=None)
def _chunk_sort_scn(limit, offset):
    """The same sort over the generator's rows bound as one chunk."""
    from tests.test_oracle_q1 import pull_lineitem
    rows = [tuple(r) for r in pull_lineitem(load_oracle(), N_SORT)]

    def plan(b, lib, srcs, is_oracle):
        return (b.topn(srcs[0], [b.colref(c, t, f) for c, t, f in KEYS_2],
                       SORT_DESC, limit, offset),
                P.LINEITEM_TYPES, P.LINEITEM_FRACS)

    return Scn(f"reopen-chunk-sort-{limit}-{offset}",
               [(P.LINEITEM_TYPES, P.LINEITEM_FRACS, rows)], plan, [],
               ordered=True)


def test_oracle_chunk_sort():
    for limit, offset in SLICES:
        _assert_sorted_same(_want(_chunk_sort_scn(limit, offset)),
                            _want_sort(limit, offset))


@pytest.mark.gpu
@pytest.mark.parametrize("limit,offset", SLICES)
def test_reopen_sort_chunks(limit, offset, monkeypatch):
    from tests.test_null_slots import _run
    scn = _chunk_sort_scn(limit, offset)
    monkeypatch.delenv("GX_SORT_RUN_ROWS", raising=False)
    monkeypatch.delenv("GX_HBM_BUDGET", raising=False)
    for rows in _run(load_product(), scn, "zero", False, 3):
        _assert_sorted_same(rows, _want(scn))


# ---------------------------------------------------- keyless LIMIT/OFFSET ---

LIMIT_ROWS = [(i, (i * 7) % 1000) for i in range(1000)]  # _run_limit's table
LIMIT_SLICES = [(5, 3), (-1, 3), (5, 5000)]


@functools.lru_cache(maxsize=None)
def _limit_scn(limit, offset, with_sel):
    def plan(b, lib, srcs, is_oracle):
        node = srcs[0]
        if with_sel:
            node = b.selection(node, [b.call(GX_F_LT, I64, 0,
                                             b.colref(1, I64),
                                             b.const_i64(500))])
        return b.topn(node, [], [], limit, offset), [I64] * 2, [0] * 2

    return Scn(f"reopen-limit-{limit}-{offset}-{with_sel}",
               [([I64] * 2, [0] * 2, LIMIT_ROWS)], plan, [], ordered=True)


def test_oracle_limit_slices():
    for with_sel in (False, True):
        kept = [r for r in LIMIT_ROWS if not with_sel or r[1] < 500]
        for limit, offset in LIMIT_SLICES:
            end = None if limit < 0 else offset + limit
            assert _want(_limit_scn(limit, offset, with_sel)) == \
                kept[offset:end]


@pytest.mark.gpu
@pytest.mark.parametrize("with_sel", [False, True])
@pytest.mark.parametrize("limit,offset", LIMIT_SLICES)
def test_reopen_keyless_limit(limit, offset, with_sel, monkeypatch):
    """Child row order preserved, so the rows compare in order."""
    _check_product(_limit_scn(limit, offset, with_sel), "zero", monkeypatch,
                   opens=3)


# ------------------------------------ sort above a Selection and a join ---

ABOVE_SLICES = {"selection": [(100, 13), (-1, 13)],
                "join": [(200, 13), (-1, 13)]}
ABOVE_SCN = {"selection": _sel_sort_scn, "join": _join_sort_scn}


@pytest.mark.parametrize("below", list(ABOVE_SCN))
def test_oracle_sort_above_slices(below):
    """The keys end in a unique id: the order is total."""
    for desc in (0, 1):
        full = _want(ABOVE_SCN[below](desc, -1, 0))
        assert len(full) > 300
        for limit, offset in ABOVE_SLICES[below]:
            end = None if limit < 0 else offset + limit
            assert _want(ABOVE_SCN[below](desc, limit, offset)) == \
                full[offset:end]


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [0, 1])
@pytest.mark.parametrize("below", list(ABOVE_SCN))
def test_reopen_sort_above(below, desc, monkeypatch):
    for limit, offset in ABOVE_SLICES[below]:
        _check_product(ABOVE_SCN[below](desc, limit, offset), "stale",
                       monkeypatch, opens=3)


# ------------------------------------ standalone Selection and Projection ---

@pytest.mark.gpu
@pytest.mark.parametrize("site", ["selection", "projection"])
def test_reopen_standalone(site, monkeypatch):
    scn = _sel_scn("or") if site == "selection" else _proj_scn("arith")
    assert len(_want(scn)) > 100
    _check_product(scn, "stale", monkeypatch, opens=3)
