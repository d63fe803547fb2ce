"""Plan routing, pinned shape by shape (CPU).

gx_build classifies the root of a plan and hands it to one compiler, or to an
ordered list of them. For every root shape the engine knows, this pins the
triple a caller can observe without a GPU: gx_open's return code, the VM site
that took the plan (the first word after `site` in gx_debug_vm_program) and
the exact gx_last_error text. Runs against the PRODUCT library: compilation
happens before the GPU check."""
import ctypes

import pytest

from tests.gxlib import (GX_AGG_COUNT, GX_AGG_COUNT_DISTINCT,
                         GX_AGG_MODE_FINAL, GX_AGG_SUM, GX_F_GT, GX_F_MUL,
                         GX_F_PLUS, GX_TYPE_DECIMAL, GX_TYPE_I64,
                         GX_TYPE_STRING, load_product)
from tidb_amd import plan as P

I64 = GX_TYPE_I64


def _c(b, i):
    return b.colref(i, I64)


def _src(b):
    return b.source([I64, I64])


def _gt0(b, col):
    return b.call(GX_F_GT, I64, 0, _c(b, col), b.const_i64(0))


def _sum01(b):
    return b.call(GX_F_PLUS, I64, 0, _c(b, 0), _c(b, 1))


def _join(b):
    """two-column sources joined on column 0: output columns 0..3"""
    return b.hashjoin(_src(b), _src(b), [_c(b, 0)], [_c(b, 0)])


COUNT = (GX_AGG_COUNT, -1, 0)


def _agg(b, child, aggs=(COUNT,), mode=0):
    """group by column 0: output = [key, aggs...]"""
    return b.hashagg(child, [_c(b, 0)], list(aggs), mode)


def _distinct(b):
    return (GX_AGG_COUNT_DISTINCT, _c(b, 1), 0)


def _top(b, child, col=1, limit=3):
    return b.topn(child, [_c(b, col)], [1], limit)


def _q3(lib, like=False):
    def like_revenue(b, rev, price, disc):
        flag = b.call(P.GX_F_LIKE, I64, 0,
                      b.colref(6 + P.L_RETFLAG, GX_TYPE_STRING),
                      b.const_str("%A%"))
        return b.call(GX_F_MUL, GX_TYPE_DECIMAL, 2, price, flag), 2
    b, _srcs, root, _t, _f = P.q3_plan(lib, wrap_revenue=like_revenue
                                       if like else None)
    return b, root


NO_JOIN_AGG = "unsupported aggregate shape for device join path"
MIXED = "DISTINCT aggregates cannot mix with plain aggregates this round"
HAVING = "unsupported HAVING condition (col cmp const, IS NULL, OR of those)"

# name -> (plan(b) -> root, open rc, site, error)
CASES = {
    "source": (lambda b: _src(b), 0, "none", ""),
    "sort_source": (lambda b: b.sort(_src(b), [_c(b, 0)], [0]),
                    0, "none", ""),
    "limit_source": (lambda b: b.topn(_src(b), [], [], 5), 0, "none", ""),
    "selection_source": (lambda b: b.selection(_src(b), [_gt0(b, 0)]),
                         0, "none", ""),
    "projection_source": (lambda b: b.projection(_src(b), [_sum01(b)]),
                          0, "projection", ""),
    "projection_selection_source": (
        lambda b: b.projection(b.selection(_src(b), [_gt0(b, 0)]),
                               [_sum01(b)]),
        0, "projection", ""),
    "hashagg_source": (lambda b: _agg(b, _src(b)), 0, "fused", ""),
    "having_hashagg": (
        lambda b: b.selection(_agg(b, _src(b)), [_gt0(b, 1)]),
        0, "fused", ""),
    "topn_hashagg": (lambda b: _top(b, _agg(b, _src(b))), 0, "fused", ""),
    "topn_having_hashagg": (
        lambda b: _top(b, b.selection(_agg(b, _src(b)), [_gt0(b, 1)])),
        0, "fused", ""),
    "final_hashagg_source": (
        lambda b: _agg(b, _src(b), mode=GX_AGG_MODE_FINAL), 0, "none", ""),
    "final_distinct": (
        lambda b: _agg(b, _src(b), [_distinct(b)], GX_AGG_MODE_FINAL),
        -1, "none", "DISTINCT aggregates support COMPLETE mode only"),
    "streamagg_sort_source": (
        lambda b: b.streamagg(b.sort(_src(b), [_c(b, 0)], [0]), [_c(b, 0)],
                              [COUNT]),
        0, "fused", ""),
    "streamagg_limited_topn": (
        lambda b: b.streamagg(b.topn(_src(b), [_c(b, 0)], [0], 5),
                              [_c(b, 0)], [COUNT]),
        -1, "none", "device streamagg expects a full-sort child this round"),
    "hashjoin": (lambda b: _join(b), 0, "none", ""),
    "selection_hashjoin": (lambda b: b.selection(_join(b), [_gt0(b, 3)]),
                           0, "none", ""),
    "topn_hashjoin": (lambda b: _top(b, _join(b), col=3), 0, "none", ""),
    "topn_selection_source": (
        lambda b: _top(b, b.selection(_src(b), [_gt0(b, 0)])),
        0, "none", ""),
    "hashagg_hashjoin": (lambda b: _agg(b, _join(b)), 0, "fused", ""),
    "having_hashagg_hashjoin": (
        lambda b: b.selection(_agg(b, _join(b)), [_gt0(b, 1)]),
        0, "fused", ""),
    # refused by the fused and the join-aggregate compilers, taken by the
    # aggregation over materialized joined rows
    "topn_hashagg_hashjoin": (lambda b: _top(b, _agg(b, _join(b))),
                              0, "fused", ""),
    "topn_having_hashagg_hashjoin": (
        lambda b: _top(b, b.selection(_agg(b, _join(b)), [_gt0(b, 1)])),
        0, "fused", ""),
    "topn_hashagg_distinct_hashjoin": (
        lambda b: _top(b, _agg(b, _join(b), [_distinct(b)])),
        0, "fused", ""),
    "topn_hashagg_mixed_distinct_hashjoin": (
        lambda b: _top(b, _agg(b, _join(b), [_distinct(b), COUNT])),
        -1, "none", MIXED),
    # a Source at the bottom: only the fused compiler can take the plan, so
    # its complaint is the one reported (before the router stopped trying
    # compilers that need a join: "expected a hash join under the
    # aggregation")
    "topn_hashagg_mixed_distinct_source": (
        lambda b: _top(b, _agg(b, _src(b), [_distinct(b), COUNT])),
        -1, "none", MIXED),
    # same rule (before: "unsupported aggregate shape for device join path")
    "topn_badkey_hashagg_source": (
        lambda b: _top(b, _agg(b, _src(b)), col=7),
        -1, "none", "sort keys must be aggregate output columns"),
    # over a join, a sort key outside the aggregate's output leaves the plan
    # to the join-aggregate compiler alone
    "topn_badkey_hashagg_hashjoin": (
        lambda b: _top(b, _agg(b, _join(b)), col=7),
        -1, "none", NO_JOIN_AGG),
    "topn_badhaving_hashagg_hashjoin": (
        lambda b: _top(b, b.selection(_agg(b, _join(b)), [_gt0(b, 7)])),
        -1, "none", HAVING),
    # recorded as they are: neither shape has an aggregate in it
    "topn_projection_source": (
        lambda b: _top(b, b.projection(_src(b), [_c(b, 0), _c(b, 1)])),
        -1, "none", NO_JOIN_AGG),
    "topn_topn_source": (lambda b: _top(b, _top(b, _src(b))),
                         -1, "none", NO_JOIN_AGG),
}

Q3_CASES = {
    "q3": (False, 0, "probe", ""),
    # the chain stops at the join-aggregate compiler's error
    "q3_value_like": (True, -1, "none",
                      "LIKE in value context is not supported in the "
                      "join-aggregate pipeline"),
}


def _lib():
    lib = load_product()
    lib.gx_debug_vm_program.restype = ctypes.c_char_p
    lib.gx_debug_vm_program.argtypes = [ctypes.c_void_p]
    return lib


def _observe(lib, b, root):
    ex = b.build(root)
    rc = lib.gx_open(ex.ex)
    prog = lib.gx_debug_vm_program(ex.ex).decode()
    err = ex.error()
    ex.free()
    b.free()
    assert prog.startswith("site "), prog
    return rc, prog.split()[1], err, prog


@pytest.mark.parametrize("name", list(CASES))
def test_route(name):
    plan, rc, site, err = CASES[name]
    lib = _lib()
    b = P.Builder(lib)
    assert _observe(lib, b, plan(b))[:3] == (rc, site, err)


@pytest.mark.parametrize("name", list(Q3_CASES))
def test_route_q3(name):
    like, rc, site, err = Q3_CASES[name]
    lib = _lib()
    b, root = _q3(lib, like)
    assert _observe(lib, b, root)[:3] == (rc, site, err)


@pytest.mark.parametrize("aggs", ["plain", "distinct"])
def test_fallback_compiles_what_the_direct_route_compiles(aggs):
    """TopN <- HashAgg <- HashJoin reaches the aggregation over joined rows
    as the third compiler tried; HashAgg <- HashJoin reaches it directly. Both
    must hold the same program: nothing an earlier attempt did to the plan
    (the DISTINCT rewrite edits the aggregate node) may reach a later one."""
    lib = _lib()
    progs = []
    for sorted_ in (False, True):
        b = P.Builder(lib)
        agg = _agg(b, _join(b), [_distinct(b)] if aggs == "distinct"
                   else [COUNT, (GX_AGG_SUM, _c(b, 3), 0)])
        rc, site, err, prog = _observe(lib, b,
                                       _top(b, agg) if sorted_ else agg)
        assert (rc, site, err) == (0, "fused", "")
        progs.append(prog)
    assert progs[0] == progs[1]
