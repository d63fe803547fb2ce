"""Oracle TPC-H Q3 end-to-end (3-table HashJoin + HashAgg + TopN) against an
independent pure-Python computation on the same synthetic rows."""
from fractions import Fraction

from tests.gxlib import (GX_TPCH_CUSTOMER, GX_TPCH_LINEITEM, GX_TPCH_ORDERS,
                         load_oracle)
from tidb_amd import plan as P

N_LI = 40000
N_ORD = N_LI // 4
N_CUST = max(N_ORD // 10, 1)

DATE_CUT = (1995 << 50) | (3 << 46) | (15 << 41)


def pull_table(lib, src_builder, types, fracs, table, n, caps):
    b = P.Builder(lib)
    src = b.source(types, fracs)
    ex = b.build(src)
    ex.bind_tpch(src, table, n)
    ex.open()
    rows = ex.pull_all(types, fracs, data_caps=caps)
    ex.close()
    ex.free()
    b.free()
    return rows


def expected_q3(lib):
    cust = pull_table(lib, None, P.CUSTOMER_TYPES, None, GX_TPCH_CUSTOMER,
                      N_CUST, [None, 65536])
    orders = pull_table(lib, None, P.ORDERS_TYPES, None, GX_TPCH_ORDERS,
                        N_ORD, [None] * 4)
    li = pull_table(lib, None, P.LINEITEM_TYPES, P.LINEITEM_FRACS,
                    GX_TPCH_LINEITEM, N_LI, [None] * 5 + [4096, 4096, None])
    building = {r[0] for r in cust if r[1] == "BUILDING"}
    ordmap = {}
    for (okey, ckey, odate, prio) in orders:
        if (odate & ~0xF) < DATE_CUT and ckey in building:
            ordmap[okey] = (odate, prio)
    groups = {}
    for r in li:
        okey, _q, price, disc, _t, _rf, _ls, sdate = r
        if (sdate & ~0xF) <= DATE_CUT:
            continue
        o = ordmap.get(okey)
        if o is None:
            continue
        pc = int(Fraction(price) * 100)
        dc = int(Fraction(disc) * 100)
        rev = pc * (100 - dc)  # scale 4 units
        key = (okey, o[0], o[1])
        groups[key] = groups.get(key, 0) + rev
    rows = [(okey, odate, prio, rev) for (okey, odate, prio), rev in groups.items()]
    # TopN: revenue desc, orderdate asc (masked-u64 compare), limit 10
    rows.sort(key=lambda r: (-r[3], r[1] & ~0xF))
    return rows[:10]


def run_q3(lib, limit=10, wrap_revenue=None):
    b, (cust, orders, li), topn, out_types, out_fracs = P.q3_plan(
        lib, limit, wrap_revenue)
    ex = b.build(topn)
    ex.bind_tpch(cust, GX_TPCH_CUSTOMER, N_CUST)
    ex.bind_tpch(orders, GX_TPCH_ORDERS, N_ORD)
    ex.bind_tpch(li, GX_TPCH_LINEITEM, N_LI)
    ex.open()
    rows = ex.pull_all(out_types, out_fracs, data_caps=[None] * 4)
    ex.close()
    ex.free()
    b.free()
    return rows


def test_q3_oracle_vs_python(oracle_lib):
    got = run_q3(oracle_lib)
    want = expected_q3(oracle_lib)
    assert len(got) == len(want) > 0
    got_cmp = [(r[0], r[1], r[2], int(Fraction(r[3]) * 10**4)) for r in got]
    # ties in (revenue, orderdate) may order differently; compare sort-key
    # multisets then exact prefix where keys are strict
    assert got_cmp == want, (got_cmp[:3], want[:3])
