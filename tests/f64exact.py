"""Inputs, exact references and derived error bounds for device f64 SUM/AVG
(tests/test_float_aggs_exact.py). Nothing here is measured on a GPU.

Three classes of f64 input, each with a reference of its own:

1. INTEGER-VALUED: every non-NULL value is an integer with |x| <= 2^20 and a
   group holds at most 2^12 of them, so every partial sum in any order is an
   integer below 2^53: exact. SUM is the Python integer sum, bit for bit, and
   AVG is float(sum) / float(count), one correctly rounded division.
2. RANDOM MANTISSA: +-m * 2^e, m a random 53-bit mantissa in [1, 2), e in
   0..16, at most 2048 non-NULL values per group, one group of cancelling
   pairs x, -x + d. The reference is the exact Fraction sum s; any summation
   tree satisfies |got - s| <= gamma(n-1) * sum|x| with gamma(k) =
   k*u / (1 - k*u), u = 2^-53 (Higham, Accuracy and Stability, section 4.2).
   The zeros of table initialisation, empty LDS partials and empty banks add
   exactly and contribute no term. For AVG one more rounding:
   gamma(n-1) * sum|x| / c + 2^-52 * |s / c|.
3. SPECIAL VALUES (SPECIAL_KINDS): the result follows from IEEE rules in any
   order, see special_sum.

Inputs are filled with numpy straight into PyColumn.data / null_bitmap; keys
are laid out as i % ndv, so that every block of 256 consecutive rows meets
min(ndv, 256) keys.
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np

from tests.gxlib import (GX_TYPE_DECIMAL, GX_TYPE_F64, GX_TYPE_I64,
                         GX_TYPE_STRING, GX_TYPE_TIME, load_oracle)
from tests.nullslots import fill_null_slots
from tidb_amd.chunkpy import PyChunk
from tidb_amd.decimals import decimal_bytes_to_str, str_to_decimal_bytes

I64, F64, DEC, TIME, STR = (GX_TYPE_I64, GX_TYPE_F64, GX_TYPE_DECIMAL,
                            GX_TYPE_TIME, GX_TYPE_STRING)

# the one input schema; a BASIC input stops after F
K, F, K2, F2, A, B, C, DK, TK, SK = range(10)
SCHEMA = [(I64, 0), (F64, 0), (I64, 0), (F64, 0), (DEC, 2), (DEC, 4),
          (DEC, 0), (DEC, 2), (TIME, 0), (STR, 0)]
BASIC, FULL = 2, len(SCHEMA)

INT_MAX_ABS = 1 << 20
INT_MAX_ROWS = 1 << 12
RAND_MAX_ROWS = 2048
U = Fraction(1, 1 << 53)

DK_LUT = ["-1.50", "0.00", "2.25", "10.75", "-0.25"]
A_LUT = ["0.00", "1.25", "-1.25", "999.99", "-999.99", "12345.67", "-0.01",
         "77.70", "-4096.00", "3.14", "-2.72", "100000.00", "0.50", "-0.50",
         "42.42", "-31337.00"]
B_LUT = ["1.0000", "-2.5000", "0.0001", "-0.0001", "33.3333", "7.0000",
         "-999.9999", "0.5000", "12.2500"]
C_LUT = ["3", "-7", "0", "11", "1", "-2", "0", "49"]
# |a * b| ~ 8e35 units at frac 6: past int64, inside int128
A_BIG = ["9000000000000000.37", "-9000000000000000.37"]
B_BIG = "90000000000000.9999"

class _Any:
    """Equal to everything: a result column the reference leaves open."""
    __hash__ = None

    def __eq__(self, other):
        return True

    def __repr__(self):
        return "ANY"


ANY = _Any()


# ---- group keys as functions of the group id --------------------------------

def key_k(g):
    return 3 * int(g) + 7  # non-negative and below 2^31: a packed key lane


def key_k2(g):
    return int(g) % 7


def key_dk(g):
    return DK_LUT[int(g) % 5]


def key_tk_date(g):
    q = int(g) // 5
    return 1995 + q // 336, 1 + q % 12, 1 + (q // 12) % 28


def key_sk(g):
    g = int(g)  # every fourth string is longer than the 16-byte inline prefix
    return f"group-key-{g:05d}-tail" if g % 4 == 0 else f"g{g:05d}"


@functools.lru_cache(maxsize=None)
def _dec40(s):
    return str_to_decimal_bytes(load_oracle(), s)


def _time(y, m, d):
    return int(load_oracle().gx_time_from_date(y, m, d))


def key_value(col, g):
    """The value a result row holds for key column `col` of group g."""
    if col == K:
        return key_k(g)
    if col == K2:
        return key_k2(g)
    if col == DK:
        return decimal_bytes_to_str(_dec40(key_dk(g)))
    if col == TK:
        v = _time(*key_tk_date(g))
        return v - (1 << 64) if v >= 1 << 63 else v
    assert col == SK
    return key_sk(g)


class Input:
    """n rows over group ids gid (= i % ndv unless sliced). f / f2 are the
    two f64 columns with their NOT-NULL masks; `tail` rows at the end carry
    A_BIG / B_BIG, whose product overflows the int64 VM."""

    def __init__(self, ndv, gid, f, fvalid, width=BASIC, f2=None,
                 f2valid=None, tail=0):
        self.ndv, self.gid, self.n = ndv, gid, len(gid)
        self.f, self.fvalid, self.width, self.tail = f, fvalid, width, tail
        self.f2 = f if f2 is None else f2
        self.f2valid = fvalid if f2valid is None else f2valid

    def slice(self, lo, hi):
        return Input(self.ndv, self.gid[lo:hi], self.f[lo:hi],
                     self.fvalid[lo:hi], self.width, self.f2[lo:hi],
                     self.f2valid[lo:hi])

    def kvals(self):
        return 3 * self.gid + 7

    def schema(self):
        return ([t for t, _ in SCHEMA[:self.width]],
                [fr for _, fr in SCHEMA[:self.width]])

    def chunk(self, mode):
        """A PyChunk of the input with the bytes under its NULLs rewritten
        as tests.nullslots mode `mode`."""
        n, gid = self.n, self.gid
        types, fracs = self.schema()
        strs = [key_sk(g).encode() for g in gid] if self.width > SK else []
        caps = [max(sum(map(len, strs)), 1) if t == STR else None
                for t in types]
        ch = PyChunk(types, max(n, 1), fracs, caps)

        def put(c, raw, valid=None, elem=8):
            col = ch.columns[c]
            col.data[:n * elem] = np.ascontiguousarray(raw).view(
                np.uint8).reshape(-1)
            if valid is not None:
                bits = np.packbits(valid, bitorder="little")
                col.null_bitmap[:len(bits)] = bits
            col.length = n

        def dec(c, lut, idx):
            table = np.stack([np.frombuffer(_dec40(s), dtype=np.uint8)
                              for s in lut])
            put(c, table[idx], elem=40)

        put(K, self.kvals().astype(np.int64))
        put(F, self.f.astype(np.float64), self.fvalid)
        if self.width > BASIC:
            i = np.arange(n)
            big = i >= n - self.tail
            put(K2, (gid % 7).astype(np.int64))
            put(F2, self.f2.astype(np.float64), self.f2valid)
            dec(A, A_LUT + A_BIG,
                np.where(big, len(A_LUT) + i % 2, (i * 7) % len(A_LUT)))
            dec(B, B_LUT + [B_BIG],
                np.where(big, len(B_LUT), (i * 5) % len(B_LUT)))
            dec(C, C_LUT, (i * 3) % len(C_LUT))
            dec(DK, DK_LUT, gid % 5)
            times = {q: _time(*key_tk_date(5 * q))
                     for q in np.unique(gid // 5).tolist()}
            put(TK, np.array([times[q] for q in (gid // 5).tolist()],
                             dtype=np.uint64))
            col = ch.columns[SK]
            col.offsets[1:n + 1] = np.cumsum([len(s) for s in strs])
            blob = b"".join(strs)
            col.data[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            col.length = n
        fill_null_slots(ch, mode)
        return ch


def i64_chunk(*cols):
    """A chunk of non-NULL int64 columns (the build side of the join)."""
    n = len(cols[0])
    ch = PyChunk([I64] * len(cols), max(n, 1))
    for c, vals in enumerate(cols):
        ch.columns[c].data[:n * 8] = np.asarray(vals, dtype=np.int64).view(
            np.uint8)
        ch.columns[c].length = n
    return ch


# ---- the three input classes ------------------------------------------------

def _gid(n, ndv):
    return np.arange(n, dtype=np.int64) % ndv


def _null_groups(gid, valid):
    """About one group in seven has every f NULL."""
    return valid & (gid % 7 != 3)


@functools.lru_cache(maxsize=None)
def int_input(n, ndv, nulls=0.1, width=BASIC, tail=0, seed=1):
    """Class 1. nulls = 0 gives a table without a NULL anywhere (sharedCnt)."""
    rng = np.random.default_rng([seed, n, ndv])
    gid = _gid(n, ndv)

    def column():
        v = rng.integers(-INT_MAX_ABS, INT_MAX_ABS + 1, n).astype(np.float64)
        valid = rng.random(n) >= nulls
        return v, (_null_groups(gid, valid) if nulls else valid)

    f, fvalid = column()
    f2, f2valid = column()
    if nulls:  # f2 has its all-NULL groups elsewhere
        f2valid = (rng.random(n) >= nulls) & (gid % 7 != 5)
    return Input(ndv, gid, f, fvalid, width, f2, f2valid, tail)


@functools.lru_cache(maxsize=None)
def random_input(n, ndv, seed=2):
    """Class 2; group 1 is the cancelling one and has no NULL."""
    rng = np.random.default_rng([seed, n, ndv])
    gid = _gid(n, ndv)

    def mant(size):  # 53-bit mantissas in [1, 2)
        return 1.0 + rng.integers(0, 1 << 52, size).astype(np.float64) / \
            float(1 << 52)

    f = np.ldexp(mant(n), rng.integers(0, 17, n).astype(np.int32))
    f *= np.where(rng.random(n) < 0.5, -1.0, 1.0)
    valid = _null_groups(gid, rng.random(n) >= 0.1)
    rows = np.flatnonzero(gid == 1)
    d = mant(len(rows)) * np.where(rng.random(len(rows)) < 0.5, -1.0, 1.0)
    x = np.ldexp(mant(len(rows)), 16)
    for j, i in enumerate(rows):
        if j % 2 == 0:
            f[i] = x[j] if j + 1 < len(rows) else d[j]
        else:
            f[i] = -x[j - 1] + d[j]
    valid[rows] = True
    return Input(ndv, gid, f, valid)


SPECIAL_KINDS = ("nan", "+inf", "-inf", "both-inf", "zeros", "subnormal",
                 "subnormal+int")
TINY = 2.0 ** -1074


def special_kind(g, shift):
    return SPECIAL_KINDS[(int(g) + shift) % len(SPECIAL_KINDS)]


@functools.lru_cache(maxsize=None)
def special_input(n, ndv, shift=0):
    """Class 3: group g is of kind SPECIAL_KINDS[(g + shift) % 7]. r is a
    row's ordinal inside its group; every group needs r up to 2."""
    gid = _gid(n, ndv)
    r = np.arange(n) // ndv
    ints = ((r * 5) % 17 - 8).astype(np.float64)
    kind = (gid + shift) % len(SPECIAL_KINDS)
    f = ints.copy()
    f[(kind == 0) & (r == 1)] = np.nan
    f[(kind == 1) & (r == 1)] = np.inf
    f[(kind == 2) & (r == 1)] = -np.inf
    f[(kind == 3) & (r == 1)] = np.inf
    f[(kind == 3) & (r == 2)] = -np.inf
    f[kind == 4] = np.where(r % 3 == 1, 0.0, -0.0)[kind == 4]
    tiny = ((r * 37) % 101 - 50).astype(np.float64) * TINY
    f[kind == 5] = tiny[kind == 5]
    # positive integers absorb the subnormals next to them in every order
    mixed = np.where(r % 2 == 0, 1.0 + (r % 5), tiny)
    f[kind == 6] = mixed[kind == 6]
    valid = (r % 8 != 5) | (r < 3)
    return Input(ndv, gid, f, valid)


# ---- references -------------------------------------------------------------

def special_sum(xs):
    """The f64 sum of xs in ANY order, for inputs whose finite partial sums
    are all exact (or, kind 'subnormal+int', absorbed the same way in every
    order): NaN wins, opposite infinities give NaN, one infinity stays, and
    a zero sum is +0.0 because every accumulator starts from zero bits and
    +0 + -0 = +0."""
    if any(x != x for x in xs):
        return float("nan")
    pos, neg = float("inf") in xs, float("-inf") in xs
    if pos or neg:
        return float("nan") if pos and neg else float("inf" if pos else "-inf")
    s = sum(map(Fraction, xs), Fraction(0))
    return float(s) if s else 0.0  # float(Fraction) rounds correctly


def group_lists(gid, ndv, vals, valid):
    out = [[] for _ in range(ndv)]
    for g, x in zip(gid[valid].tolist(), vals[valid].tolist()):
        out[g].append(x)
    return out


def is_int_class(v):
    return bool(len(v) == 0 or (np.isfinite(v).all() and
                                (v == np.rint(v)).all() and
                                np.abs(v).max() <= INT_MAX_ABS))


def exact_sums(gid, ndv, vals, valid):
    """(sum per group or None, non-NULL count per group)."""
    cnt = np.bincount(gid[valid], minlength=ndv)
    v, g = vals[valid], gid[valid]
    if is_int_class(v):
        acc = np.zeros(ndv, dtype=np.int64)
        np.add.at(acc, g, v.astype(np.int64))
        sums = [float(int(a)) for a in acc]  # integers below 2^53
    else:
        sums = [special_sum(xs) for xs in group_lists(gid, ndv, vals, valid)]
    return [s if c else None for s, c in zip(sums, cnt.tolist())], cnt


def gamma(k):
    return k * U / (1 - k * U)


class GroupStats:
    """Exact figures of one group of class 2."""

    def __init__(self, xs):
        fr = [Fraction(x) for x in xs]
        self.n = len(fr)
        self.s = sum(fr, Fraction(0))
        self.abs = sum(map(abs, fr), Fraction(0))
        self.min_abs = min(map(abs, fr)) if fr else None

    def sum_bound(self):
        return gamma(self.n - 1) * self.abs

    def avg_bound(self):
        return (self.sum_bound() / self.n +
                Fraction(1, 1 << 52) * abs(self.s / self.n))


def fraction_stats(inp):
    return [GroupStats(xs) for xs in
            group_lists(inp.gid, inp.ndv, inp.f, inp.fvalid)]


def reference(inp, keys, aggs, rowmask=None, times=None):
    """The rows of `aggs GROUP BY keys` over the rows in rowmask, sorted as
    sort_rows does. An aggregate is ("sum" | "avg" | "count", F | F2),
    ("count*",) or ("x", ...), which the reference leaves open (ANY).
    times[g] repeats each row of group g (rows multiplied by a join)."""
    grouped = bool(keys)
    gid = inp.gid if grouped else np.zeros(inp.n, dtype=np.int64)
    ndv = inp.ndv if grouped else 1
    mask = np.ones(inp.n, dtype=bool) if rowmask is None else rowmask
    times = [1] * ndv if times is None else times
    star = np.bincount(gid[mask], minlength=ndv).tolist()
    cols = {}
    for c, (vals, valid) in ((F, (inp.f, inp.fvalid)),
                             (F2, (inp.f2, inp.f2valid))):
        if any(len(a) > 1 and a[0] != "x" and a[1] == c for a in aggs):
            cols[c] = exact_sums(gid, ndv, vals, valid & mask)
    rows = []
    for g in range(ndv):
        t = times[g]
        if star[g] * t == 0 and grouped:
            continue
        row = [key_value(c, g) for c in keys]
        for a in aggs:
            if a[0] == "count*":
                row.append(star[g] * t)
            elif a[0] == "x":
                row.append(ANY)
            else:
                sums, cnt = cols[a[1]]
                s, c = sums[g], int(cnt[g])
                if s is not None and t != 1:
                    s = special_sum([s] * t)
                if a[0] == "count":
                    row.append(c * t)
                elif a[0] == "sum":
                    row.append(s)
                else:
                    row.append(None if s is None else s / float(c * t))
        rows.append(tuple(row))
    return sort_rows(rows, len(keys))


# ---- results ----------------------------------------------------------------

NAN_BITS = 0x7FF8000000000000


def fbits(x):
    """A double as its bits, every NaN as one NaN: what 'bit for bit, any NaN
    equal to any NaN' compares."""
    if x != x:
        return ("f64", NAN_BITS)
    return ("f64", int(np.float64(x).view(np.uint64)))


def canon(rows):
    return [tuple(fbits(v) if isinstance(v, float) else v for v in r)
            for r in rows]


def sort_rows(rows, nkeys):
    return sorted(rows, key=lambda r: repr(r[:nkeys]))


def pull(ex, out_types, out_fracs):
    """Executor.pull_all with the fixed-width columns decoded by numpy; f64
    cells come back as Python floats, NULLs as None."""
    caps = [64 * 1024 if t == STR else None for t in out_types]
    chunk = PyChunk(out_types, 1024, out_fracs, caps)
    rows = []
    while True:
        for col in chunk.columns:
            col.length = 0
        g = chunk.as_gx()
        n = ctypes.c_int32(0)
        rc = ex.lib.gx_next(ex.ex, ctypes.byref(g), ctypes.byref(n))
        assert rc == 0, f"next failed ({rc}): {ex.error()}"
        n = n.value
        if n == 0:
            return rows
        cols = []
        for c, col in enumerate(chunk.columns):
            col.length = g.cols[c].length
            if col.typ in (DEC, STR):
                cols.append([chunk.cell(c, i) for i in range(n)])
                continue
            raw = col.data[:n * 8].view(
                np.float64 if col.typ == F64 else np.int64).tolist()
            ok = np.unpackbits(col.null_bitmap[:(n + 7) // 8],
                               bitorder="little")[:n].tolist()
            cols.append([v if k else None for v, k in zip(raw, ok)])
        rows.extend(zip(*cols))
