// Host-only check of the result stage (tidb_amd/csrc/gx_result.{h,cpp}): the
// two compares, the SUM/AVG finalizer, the DISTINCT fold, HAVING, ORDER BY /
// LIMIT, chunk emission and the FINAL merge, each against a reference written
// here. Stand-alone: needs no GPU, no HIP and no Python. Output buffers are
// heap blocks of exactly the stated capacity, so ASan sees any overrun.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I tidb_amd/csrc \
//       -I include tools/result_stage_check.cpp tidb_amd/csrc/gx_result.cpp \
//       tidb_amd/csrc/gx_decimal.cpp -o result_stage_check
//   ./result_stage_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gx_result.h"

using namespace gxp;

static int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      failures++;                                                    \
    }                                                                \
  } while (0)

// ---------------- value builders and an integer decimal reference ----------

typedef __int128 i128;

static i128 pow10(int n) {
  i128 p = 1;
  while (n-- > 0) p *= 10;
  return p;
}

// units at `scale` as text with exactly `scale` fraction digits
static std::string unitsText(i128 u, int scale) {
  bool neg = u < 0;
  unsigned __int128 a = neg ? -(unsigned __int128)u : (unsigned __int128)u;
  std::string digits;
  do {
    digits.insert(digits.begin(), (char)('0' + (int)(a % 10)));
    a /= 10;
  } while (a);
  while ((int)digits.size() <= scale) digits.insert(digits.begin(), '0');
  if (scale) digits.insert(digits.end() - scale, '.');
  return (neg ? "-" : "") + digits;
}

// half-up (half away from zero) to `frac` digits, exact
static i128 roundUnits(i128 u, int scale, int frac) {
  if (frac >= scale) return u * pow10(frac - scale);
  i128 div = pow10(scale - frac);
  i128 a = u < 0 ? -u : u;
  i128 q = a / div + (2 * (a % div) >= div ? 1 : 0);
  return u < 0 ? -q : q;
}

static MyDecimal decOf(const std::string& s) {
  MyDecimal d;
  int32_t ec = d.FromString(s.data(), (int)s.size());
  CHECK(ec == E_OK);
  return d;
}

static OutRowVal I(int64_t x) {
  OutRowVal v;
  v.type = GX_TYPE_I64;
  v.i64 = x;
  v.u64 = (uint64_t)x;
  return v;
}
static OutRowVal F(double x) {
  OutRowVal v;
  v.type = GX_TYPE_F64;
  v.f64 = x;
  return v;
}
static OutRowVal T(uint64_t x) {
  OutRowVal v;
  v.type = GX_TYPE_TIME;
  v.u64 = x;
  v.i64 = (int64_t)x;
  return v;
}
static OutRowVal S(const std::string& x) {
  OutRowVal v;
  v.type = GX_TYPE_STRING;
  v.str = x;
  return v;
}
// a decimal cell; its units ride along in i64 (which the stage never reads
// for a DECIMAL) so the references below can work in integers
static OutRowVal D(int64_t units, int scale) {
  OutRowVal v;
  v.type = GX_TYPE_DECIMAL;
  v.dec = decOf(unitsText(units, scale));
  v.i64 = units;
  return v;
}
static OutRowVal N(int type) {
  OutRowVal v;
  v.type = type;
  v.isNull = true;
  return v;
}

static int sign(int c) { return c < 0 ? -1 : (c > 0 ? 1 : 0); }

// value check of a decimal cell against units at `scale`
static bool decIs(const OutRowVal& v, i128 units, int scale) {
  return v.type == GX_TYPE_DECIMAL && !v.isNull && v.dec.digitsFrac == scale &&
         v.dec.Compare(decOf(unitsText(units, scale))) == 0;
}

// ---------------- compares ----------------

static void checkCompares() {
  struct Pair {
    OutRowVal a, b;
    int order, identity;  // expected sign of cmp(a, b)
  };
  const uint64_t t0 = 0x1F4A5B6C7D8E9F00ULL;
  const std::vector<Pair> pairs = {
      {I(-5), I(3), -1, -1},
      {I(7), I(7), 0, 0},
      {I(INT64_MIN), I(INT64_MAX), -1, -1},
      {F(-0.5), F(0.25), -1, -1},
      {F(2.0), F(2.0), 0, 0},
      {D(-125, 2), D(100, 2), -1, -1},
      {D(150, 2), D(15, 1), 0, 0},
      {T(t0), T(t0 + 0x10), -1, -1},
      {T(t0 | 0x3), T(t0 | 0xC), 0, -1},  // differ in the low 4 bits only
      {S("a"), S("b"), -1, -1},
      {S("a"), S("a "), 0, -1},  // PAD SPACE
      {S("a  "), S("a "), 0, 1},
      {S("a "), S("a!"), -1, -1},
      {S(""), S("   "), 0, -1},
      {N(GX_TYPE_I64), I(INT64_MIN), -1, -1},
      {N(GX_TYPE_STRING), S(""), -1, -1},
      {N(GX_TYPE_DECIMAL), D(-1, 0), -1, -1},
      {N(GX_TYPE_TIME), N(GX_TYPE_TIME), 0, 0},
  };
  for (const Pair& p : pairs) {
    CHECK(sign(cmpOrder(p.a, p.b)) == p.order);
    CHECK(sign(cmpOrder(p.b, p.a)) == -p.order);
    CHECK(sign(cmpIdentity(p.a, p.b)) == p.identity);
    CHECK(sign(cmpIdentity(p.b, p.a)) == -p.identity);
    CHECK(cmpOrder(p.a, p.a) == 0 && cmpIdentity(p.b, p.b) == 0);
  }
}

// ---------------- finalizer ----------------

static void checkFinalizer() {
  // divisors of 10^4: the quotient terminates within the four extra digits
  const int64_t counts[] = {1,   2,   4,   5,   8,    10,   16,   20,  25,
                            40,  50,  80,  100, 125,  200,  250,  400, 500,
                            625, 1000, 1250, 2000, 2500, 5000, 10000};
  std::mt19937_64 rng(11);
  std::vector<i128> sums = {0, 1, -1, 7, -7, 999999, -1000001, 123456789012345LL,
                            -987654321098765LL,
                            // needs more than 64 bits
                            (i128)1234567890123456789LL * 1000000007LL,
                            -(i128)1234567890123456789LL * 999999937LL};
  for (int i = 0; i < 40; i++) sums.push_back((i128)(int64_t)rng() / 1000);
  for (int scale : {0, 2, 4, 6}) {
    for (i128 u : sums) {
      MyDecimal sum = decFromUnits(u, scale);
      // decFromUnits itself: value and text against the integer reference
      CHECK(sum.ToString() == unitsText(u, scale));
      CHECK(sum.Compare(decOf(unitsText(u, scale))) == 0);
      for (int64_t cnt : counts) {
        const i128 avg = u * 10000 / cnt;  // exact, at scale + 4
        for (int frac : {scale + 4, scale + 2, scale, 0}) {
          for (int func : {GX_AGG_AVG, GX_AGG_AVG_DISTINCT}) {
            OutRowVal v;
            CHECK(finalizeDecimalAgg(func, sum, cnt, frac, &v));
            CHECK(decIs(v, roundUnits(avg, scale + 4, frac), frac));
          }
          for (int func : {GX_AGG_SUM, GX_AGG_SUM_DISTINCT}) {
            OutRowVal v;
            CHECK(finalizeDecimalAgg(func, sum, cnt, frac, &v));
            CHECK(decIs(v, roundUnits(u, scale, frac), frac));
          }
        }
      }
      for (int func : {GX_AGG_SUM, GX_AGG_AVG, GX_AGG_SUM_DISTINCT,
                       GX_AGG_AVG_DISTINCT}) {
        OutRowVal v;
        CHECK(finalizeDecimalAgg(func, sum, 0, scale, &v));
        CHECK(v.isNull && v.type == GX_TYPE_DECIMAL);
      }
    }
  }
  OutRowVal v;
  finalizeF64Agg(GX_AGG_SUM, 7.5, 3, &v);
  CHECK(v.type == GX_TYPE_F64 && !v.isNull && v.f64 == 7.5);
  v = OutRowVal();
  finalizeF64Agg(GX_AGG_AVG, 7.5, 3, &v);
  CHECK(v.type == GX_TYPE_F64 && !v.isNull && v.f64 == 7.5 / 3.0);
  v = OutRowVal();
  finalizeF64Agg(GX_AGG_AVG, -1.0, 0, &v);
  CHECK(v.type == GX_TYPE_F64 && v.isNull);
  v = OutRowVal();
  finalizeF64Agg(GX_AGG_SUM, 0.0, 0, &v);
  CHECK(v.isNull);
}

// ---------------- DISTINCT fold ----------------

// identity of two cells, written out here: raw bits, untrimmed strings
static bool sameCell(const OutRowVal& a, const OutRowVal& b) {
  if (a.isNull || b.isNull) return a.isNull && b.isNull;
  switch (a.type) {
    case GX_TYPE_STRING: return a.str == b.str;
    case GX_TYPE_TIME: return a.u64 == b.u64;
    default: return a.i64 == b.i64;  // I64, and DECIMAL units (see D())
  }
}

static void checkDistinctCase(const std::vector<ResultRow>& in, int nKeys) {
  // per row: keys..., then arg0 DECIMAL(scale 2), arg1 STRING
  DistinctSpec spec;
  spec.nKeys = nKeys;
  spec.funcs = {GX_AGG_COUNT_DISTINCT, GX_AGG_SUM_DISTINCT,
                GX_AGG_AVG_DISTINCT, GX_AGG_COUNT_DISTINCT};
  spec.fracs = {0, 2, 6, 0};
  spec.argSlot = {{0}, {0}, {0}, {0, 1}};
  std::vector<ResultRow> got = in;
  std::string err;
  CHECK(foldDistinct(&got, spec, &err) == GX_OK && err.empty());

  // brute force: groups in first-seen order, O(n^2) dedup per aggregate
  std::vector<ResultRow> groupKeys;
  std::vector<std::vector<const ResultRow*>> members;
  for (const ResultRow& r : in) {
    size_t g = 0;
    for (; g < groupKeys.size(); g++) {
      bool same = true;
      for (int k = 0; k < nKeys; k++) same &= sameCell(groupKeys[g][k], r[k]);
      if (same) break;
    }
    if (g == groupKeys.size()) {
      groupKeys.emplace_back(r.begin(), r.begin() + nKeys);
      members.emplace_back();
    }
    members[g].push_back(&r);
  }
  if (nKeys == 0 && groupKeys.empty()) {  // scalar default row
    groupKeys.emplace_back();
    members.emplace_back();
  }
  CHECK(got.size() == groupKeys.size());
  if (got.size() != groupKeys.size()) return;
  for (size_t g = 0; g < groupKeys.size(); g++) {
    const ResultRow& row = got[g];
    CHECK(row.size() == (size_t)nKeys + 4);
    if (row.size() != (size_t)nKeys + 4) return;
    for (int k = 0; k < nKeys; k++) {
      CHECK(sameCell(row[k], groupKeys[g][k]));
      CHECK(row[k].type == groupKeys[g][k].type);
    }
    std::vector<const OutRowVal*> d0;  // distinct non-NULL arg0
    std::vector<const ResultRow*> d01;  // distinct all-non-NULL (arg0, arg1)
    for (const ResultRow* r : members[g]) {
      const OutRowVal& a0 = (*r)[nKeys];
      const OutRowVal& a1 = (*r)[nKeys + 1];
      bool seen = a0.isNull;
      for (const OutRowVal* p : d0) seen |= sameCell(*p, a0);
      if (!seen) d0.push_back(&a0);
      seen = a0.isNull || a1.isNull;
      for (const ResultRow* p : d01)
        seen |= sameCell((*p)[nKeys], a0) && sameCell((*p)[nKeys + 1], a1);
      if (!seen) d01.push_back(r);
    }
    i128 sum = 0;
    for (const OutRowVal* p : d0) sum += p->i64;
    const int64_t cnt = (int64_t)d0.size();
    const OutRowVal* v = &row[nKeys];
    CHECK(v[0].type == GX_TYPE_I64 && !v[0].isNull && v[0].i64 == cnt);
    CHECK(v[3].type == GX_TYPE_I64 && !v[3].isNull &&
          v[3].i64 == (int64_t)d01.size());
    if (cnt == 0) {
      CHECK(v[1].isNull && v[1].type == GX_TYPE_DECIMAL);
      CHECK(v[2].isNull && v[2].type == GX_TYPE_DECIMAL);
    } else {
      CHECK(decIs(v[1], sum, 2));
      // the pool's values are multiples of 3.00 and cnt <= 4: exact at 6
      CHECK(sum * 10000 % cnt == 0);
      CHECK(decIs(v[2], sum * 10000 / cnt, 6));
    }
  }
}

static void checkDistinct() {
  std::mt19937 rng(5);
  const int64_t pool[4] = {300, 600, -900, 1200};
  const char* strs[4] = {"a", "a ", "b", ""};
  for (int nKeys : {1, 0}) {
    for (int rows : {0, 1, 48}) {
      std::vector<ResultRow> in;
      for (int i = 0; i < rows; i++) {
        ResultRow r;
        if (nKeys) {
          int k = (int)(rng() % 5);
          r.push_back(k == 4 ? N(GX_TYPE_I64) : I(k * 1000 - 1000));
        }
        int a = (int)(rng() % 6);
        r.push_back(a >= 4 ? N(GX_TYPE_DECIMAL) : D(pool[a], 2));
        int s = (int)(rng() % 5);
        r.push_back(s == 4 ? N(GX_TYPE_STRING) : S(strs[s]));
        in.push_back(std::move(r));
      }
      checkDistinctCase(in, nKeys);
    }
  }
  // a group whose every argument is NULL keeps its row
  checkDistinctCase({{I(1), N(GX_TYPE_DECIMAL), N(GX_TYPE_STRING)},
                     {I(2), D(300, 2), S("x")},
                     {I(1), N(GX_TYPE_DECIMAL), S("y")}},
                    1);
}

// ---------------- HAVING ----------------

static HavingLeaf leaf(int col, int cmp, const OutRowVal& cst) {
  HavingLeaf l;
  l.col = col;
  l.cmp = cmp;
  l.cst = cst;
  return l;
}
static HavingLeaf nullLeaf(int col, bool wantNull) {
  HavingLeaf l;
  l.col = col;
  l.isNullTest = true;
  l.wantNull = wantNull;
  return l;
}

static bool refCmp(int cmp, int c) {
  switch (cmp) {
    case GX_F_LT: return c < 0;
    case GX_F_LE: return c <= 0;
    case GX_F_GT: return c > 0;
    case GX_F_GE: return c >= 0;
    case GX_F_EQ: return c == 0;
    default: return c != 0;
  }
}

static void checkHaving() {
  const uint64_t t0 = 0x1F4A5B6C7D8E9F00ULL;
  struct Case {
    OutRowVal v, cst;
    int c;  // reference 3-way result of v against cst
  };
  const std::vector<Case> cases = {
      {D(-150, 2), D(5, 1), -1}, {D(50, 2), D(5, 1), 0}, {D(51, 2), D(5, 1), 1},
      {I(-3), I(4), -1},         {I(4), I(4), 0},        {I(5), I(4), 1},
      {T(t0), T(t0 + 0x10), -1}, {T(t0 | 5), T(t0 | 9), 0},
      {T(t0 + 0x20), T(t0 + 0x1F), 1},
      {S("ab"), S("b"), -1},     {S("b  "), S("b"), 0},  {S("c"), S("b "), 1},
  };
  const int cmps[6] = {GX_F_LT, GX_F_LE, GX_F_GT, GX_F_GE, GX_F_EQ, GX_F_NE};
  for (const Case& k : cases) {
    for (int cmp : cmps) {
      bool typeOk = true;
      bool pass = havingPass({I(0), k.v}, {{leaf(1, cmp, k.cst)}}, &typeOk);
      if (k.v.type == GX_TYPE_STRING && cmp != GX_F_EQ && cmp != GX_F_NE) {
        CHECK(!typeOk);  // strings pair for = and <> only
      } else {
        CHECK(typeOk);
        CHECK(pass == refCmp(cmp, k.c));
      }
    }
  }
  // unpaired types fail, whatever the compare
  for (int cmp : cmps) {
    bool typeOk = true;
    havingPass({I(1)}, {{leaf(0, cmp, D(100, 2))}}, &typeOk);
    CHECK(!typeOk);
    typeOk = true;
    havingPass({F(1.0)}, {{leaf(0, cmp, F(1.0))}}, &typeOk);
    CHECK(!typeOk);
  }
  const ResultRow row = {N(GX_TYPE_I64), I(10), S("x")};
  const HavingLeaf onNull = leaf(0, GX_F_NE, I(99));  // NULL rejects
  const HavingLeaf yes = leaf(1, GX_F_GT, I(5));
  const HavingLeaf no = leaf(1, GX_F_LT, I(5));
  const HavingLeaf bad = leaf(1, GX_F_EQ, S("10"));  // I64 value, STRING const
  struct Expect {
    std::vector<HavingCond> conds;
    bool pass, typeOk;
  };
  const std::vector<Expect> expects = {
      {{}, true, true},
      {{{onNull}}, false, true},
      {{{onNull}, {yes}}, false, true},   // NULL under AND
      {{{yes}, {onNull}}, false, true},
      {{{onNull, yes}}, true, true},      // NULL under OR
      {{{onNull, no}}, false, true},
      {{{nullLeaf(0, true)}}, true, true},
      {{{nullLeaf(0, false)}}, false, true},
      {{{nullLeaf(1, false)}, {nullLeaf(1, true), yes}}, true, true},
      {{{yes, bad}}, true, true},         // right leaf never reached
      {{{no, bad}}, false, false},        // reached: the query fails
      {{{no}, {bad}}, false, true},       // AND stops at the first failure
      {{{yes}, {bad}}, false, false},
      {{{no, no, yes}}, true, true},      // nested OR, in order
      {{{leaf(7, GX_F_EQ, I(1))}}, false, false},  // column beyond the row
  };
  for (const Expect& e : expects) {
    bool typeOk = true;
    bool pass = havingPass(row, e.conds, &typeOk);
    CHECK(typeOk == e.typeOk);
    if (e.typeOk) CHECK(pass == e.pass);
  }
}

// ---------------- ORDER BY / LIMIT ----------------

static void checkSort() {
  std::mt19937 rng(3);
  std::vector<ResultRow> in;
  for (int i = 0; i < 60; i++) {
    int a = (int)(rng() % 5), b = (int)(rng() % 4);
    in.push_back({a == 4 ? N(GX_TYPE_I64) : I(a), b == 3 ? N(GX_TYPE_I64) : I(b),
                  I(i)});  // column 2: input position
  }
  // NULL below every value
  auto rank = [](const OutRowVal& v) { return v.isNull ? INT64_MIN : v.i64; };
  struct Keys {
    std::vector<std::pair<int, bool>> keys;
    int64_t offset, limit;
  };
  const std::vector<Keys> runs = {
      {{{0, false}}, 0, -1},              // stability on ties
      {{{0, true}}, 0, -1},               // descending, ties stay in order
      {{{0, true}, {1, false}}, 0, -1},
      {{{1, false}, {0, true}}, 7, 10},
      {{{0, false}}, 55, 10},             // limit runs past the end
      {{{0, false}}, 60, -1},             // offset at the end
      {{{0, false}}, 1000, 5},            // offset beyond the end
      {{{0, false}}, 0, 0},
      {{}, 3, 4},                         // no keys: slice only
  };
  for (const Keys& k : runs) {
    // reference: stable insertion sort, then the slice
    std::vector<ResultRow> want;
    for (const ResultRow& r : in) {
      size_t at = want.size();
      while (at > 0) {
        int c = 0;
        for (auto& [col, desc] : k.keys) {
          int64_t x = rank(want[at - 1][col]), y = rank(r[col]);
          c = x < y ? -1 : (x > y ? 1 : 0);
          if (desc) c = -c;
          if (c) break;
        }
        if (c <= 0) break;  // equal keys: the later row stays behind
        at--;
      }
      want.insert(want.begin() + at, r);
    }
    size_t b = std::min<size_t>((size_t)k.offset, want.size());
    size_t e = k.limit < 0 ? want.size()
                           : std::min<size_t>(b + (size_t)k.limit, want.size());
    std::vector<ResultRow> got = in;
    sortAndSlice(&got, k.keys, k.offset, k.limit);
    CHECK(got.size() == e - b);
    for (size_t i = 0; i < got.size() && i < e - b; i++)
      CHECK(got[i][2].i64 == want[b + i][2].i64);
  }
  std::vector<ResultRow> none;
  sortAndSlice(&none, {{0, false}}, 5, -1);
  CHECK(none.empty());
}

// ---------------- emission ----------------

// one output chunk whose every buffer has exactly the stated capacity
struct OutChunk {
  std::vector<std::unique_ptr<uint8_t[]>> blocks;
  std::vector<gx_col> cols;
  gx_chunk chunk{};
  void* block(size_t bytes) {
    blocks.emplace_back(new uint8_t[bytes ? bytes : 1]);
    std::memset(blocks.back().get(), 0xAB, bytes);
    return blocks.back().get();
  }
  void fixed(int rows, int elem, int64_t dataCap) {
    gx_col c{};
    c.data = block((size_t)dataCap);
    c.null_bitmap = (uint8_t*)block((rows + 7) / 8);
    c.elem_size = elem;
    c.data_cap = dataCap;
    cols.push_back(c);
  }
  void varlen(int rows, int64_t dataCap, int64_t offsetsCap) {
    gx_col c{};
    c.data = block((size_t)dataCap);
    c.null_bitmap = (uint8_t*)block((rows + 7) / 8);
    c.offsets = (int64_t*)block((size_t)offsetsCap * 8);
    c.elem_size = -1;
    c.data_cap = dataCap;
    c.offsets_cap = offsetsCap;
    cols.push_back(c);
  }
  gx_chunk* get() {
    chunk.cols = cols.data();
    chunk.n_cols = (int)cols.size();
    return &chunk;
  }
};

static bool nullAt(int i) { return i == 0 || i == 7 || i == 8; }

static std::vector<ResultRow> emitInput(int n) {
  std::vector<ResultRow> rows;
  for (int i = 0; i < n; i++) {
    bool nul = nullAt(i);
    rows.push_back({nul ? N(GX_TYPE_I64) : I(1000 + i),
                    nul ? N(GX_TYPE_DECIMAL) : D(i * 7 - 50, 2),
                    nul ? N(GX_TYPE_F64) : F(i * 0.5),
                    nul ? N(GX_TYPE_STRING) : S(std::string(i % 5, 'a' + i % 7)),
                    nul ? N(GX_TYPE_TIME) : T(0x1000 + (uint64_t)i * 16)});
  }
  return rows;
}

static int64_t strBytes(const std::vector<ResultRow>& rows, size_t b, size_t e) {
  int64_t n = 0;
  for (size_t i = b; i < e; i++)
    if (!rows[i][3].isNull) n += (int64_t)rows[i][3].str.size();
  return n;
}

static OutChunk exactChunk(const std::vector<ResultRow>& rows, size_t b,
                           size_t e) {
  int n = (int)(e - b);
  OutChunk oc;
  oc.fixed(n, 8, n * 8);
  oc.fixed(n, 40, n * 40);
  oc.fixed(n, 8, n * 8);
  oc.varlen(n, strBytes(rows, b, e), n + 1);
  oc.fixed(n, 8, n * 8);
  return oc;
}

static void checkEmitted(const std::vector<ResultRow>& rows, size_t b,
                         const gx_chunk* ch, int n) {
  CHECK(ch->n_rows == n && ch->n_cols == 5);
  for (int c = 0; c < 5; c++) CHECK(ch->cols[c].length == n);
  const uint8_t zeros[40] = {0};
  for (int i = 0; i < n; i++) {
    const ResultRow& r = rows[b + i];
    for (int c = 0; c < 5; c++) {
      const gx_col& g = ch->cols[c];
      bool notNull = (g.null_bitmap[i / 8] >> (i % 8)) & 1;
      CHECK(notNull == !r[c].isNull);
      if (c == 3) {
        int64_t len = g.offsets[i + 1] - g.offsets[i];
        CHECK(len == (r[c].isNull ? 0 : (int64_t)r[c].str.size()));
        if (len == (int64_t)r[c].str.size())
          CHECK(!std::memcmp((uint8_t*)g.data + g.offsets[i], r[c].str.data(),
                             (size_t)len));
        continue;
      }
      int es = c == 1 ? 40 : 8;
      const uint8_t* cell = (const uint8_t*)g.data + (size_t)i * es;
      const void* want = r[c].isNull ? (const void*)zeros
                         : c == 1    ? (const void*)&r[c].dec
                         : c == 2    ? (const void*)&r[c].f64
                                     : (const void*)&r[c].i64;
      CHECK(!std::memcmp(cell, want, es));
    }
  }
  CHECK(ch->cols[3].offsets[0] == 0);
}

static void checkEmit() {
  const std::vector<ResultRow> rows = emitInput(1025);
  size_t pos = 0;
  int32_t n = -1;
  std::string err;
  {
    OutChunk oc = exactChunk(rows, 0, 1024);
    CHECK(emitRows(rows, &pos, oc.get(), &n, &err) == GX_OK);
    CHECK(n == 1024 && pos == 1024 && err.empty());
    checkEmitted(rows, 0, oc.get(), 1024);
  }
  {
    OutChunk oc = exactChunk(rows, 1024, 1025);
    CHECK(emitRows(rows, &pos, oc.get(), &n, &err) == GX_OK);
    CHECK(n == 1 && pos == 1025);
    checkEmitted(rows, 1024, oc.get(), 1);
    n = -1;
    CHECK(emitRows(rows, &pos, oc.get(), &n, &err) == GX_OK);
    CHECK(n == 0 && pos == 1025);
  }
  // every capacity one short, one at a time: the cell that does not fit is
  // in the last row (12 rows), and that row is all NULL (9 rows)
  for (int rowsN : {12, 9}) {
    const std::vector<ResultRow> small(rows.begin(), rows.begin() + rowsN);
    const int64_t sb = strBytes(small, 0, small.size());
    for (int shortCol = 0; shortCol < 6; shortCol++) {
      OutChunk oc;
      oc.fixed(rowsN, 8, rowsN * 8 - (shortCol == 0));
      oc.fixed(rowsN, 40, rowsN * 40 - (shortCol == 1));
      oc.fixed(rowsN, 8, rowsN * 8 - (shortCol == 2));
      oc.varlen(rowsN, sb - (shortCol == 3), rowsN + 1 - (shortCol == 4));
      oc.fixed(rowsN, 8, rowsN * 8 - (shortCol == 5));
      size_t p = 0;
      err.clear();
      CHECK(emitRows(small, &p, oc.get(), &n, &err) == GX_ERR_INVALID);
      CHECK(err == "output buffer too small");
      CHECK(p == 0);
    }
  }
  {
    const std::vector<ResultRow> four(rows.begin(), rows.begin() + 4);
    OutChunk oc;
    oc.fixed(4, 8, 32);
    size_t p = 0;
    err.clear();
    CHECK(emitRows(four, &p, oc.get(), &n, &err) == GX_ERR_INVALID);
    CHECK(err == "output chunk column count mismatch");
  }
}

// ---------------- FINAL merge ----------------

static HostCol hostCol(int type, const std::vector<OutRowVal>& cells) {
  HostCol hc;
  hc.type = type;
  hc.frac = 0;
  hc.length = (int)cells.size();
  hc.nullBitmap.assign((cells.size() + 7) / 8, 0);
  if (type == GX_TYPE_STRING) hc.offsets.push_back(0);
  for (size_t i = 0; i < cells.size(); i++) {
    const OutRowVal& v = cells[i];
    if (!v.isNull) hc.nullBitmap[i / 8] |= 1 << (i % 8);
    if (type == GX_TYPE_STRING) {
      if (!v.isNull) hc.data.insert(hc.data.end(), v.str.begin(), v.str.end());
      hc.offsets.push_back((int64_t)hc.data.size());
    } else {
      const void* src = type == GX_TYPE_DECIMAL ? (const void*)&v.dec
                        : type == GX_TYPE_F64   ? (const void*)&v.f64
                                                : (const void*)&v.i64;
      size_t es = type == GX_TYPE_DECIMAL ? 40 : 8;
      const uint8_t* p = (const uint8_t*)src;
      if (v.isNull) hc.data.insert(hc.data.end(), es, 0);
      else hc.data.insert(hc.data.end(), p, p + es);
    }
  }
  return hc;
}

static void checkMergeFinal() {
  // group | COUNT | SUM(dec): sum,cnt | AVG(f64): sum,cnt | MIN(str) | FIRSTROW
  FinalSpec spec;
  spec.nGroup = 1;
  spec.funcs = {GX_AGG_COUNT, GX_AGG_SUM, GX_AGG_AVG, GX_AGG_MIN,
                GX_AGG_FIRSTROW};
  spec.fracs = {0, 2, 0, 0, 0};
  spec.argIsF64 = {0, 0, 1, 0, 0};
  std::vector<std::vector<HostCol>> chunks(2);
  // shard 0: groups "A" (shared) and "B"
  chunks[0] = {hostCol(GX_TYPE_STRING, {S("A"), S("B")}),
               hostCol(GX_TYPE_I64, {I(2), I(4)}),
               hostCol(GX_TYPE_DECIMAL, {D(125, 2), N(GX_TYPE_DECIMAL)}),
               hostCol(GX_TYPE_I64, {I(2), I(0)}),
               hostCol(GX_TYPE_F64, {F(3.0), F(0.0)}),
               hostCol(GX_TYPE_I64, {I(2), I(0)}),
               hostCol(GX_TYPE_STRING, {S("m  "), N(GX_TYPE_STRING)}),
               hostCol(GX_TYPE_I64, {N(GX_TYPE_I64), I(41)})};
  // shard 1: "A " is group "A" under PAD SPACE; "C" is private
  chunks[1] = {hostCol(GX_TYPE_STRING, {S("C"), S("A ")}),
               hostCol(GX_TYPE_I64, {I(1), I(3)}),
               hostCol(GX_TYPE_DECIMAL, {D(-5, 2), D(250, 2)}),
               hostCol(GX_TYPE_I64, {I(1), I(3)}),
               hostCol(GX_TYPE_F64, {F(-1.5), F(5.0)}),
               hostCol(GX_TYPE_I64, {I(1), I(2)}),
               hostCol(GX_TYPE_STRING, {S("m"), S("k ")}),
               hostCol(GX_TYPE_I64, {I(43), I(42)})};
  std::vector<ResultRow> rows = {{I(99)}};  // replaced, not appended to
  std::string err;
  CHECK(mergeFinal(chunks, spec, &rows, &err) == GX_OK && err.empty());
  CHECK(rows.size() == 3);
  if (rows.size() == 3) {
    const ResultRow& a = rows[0];
    const ResultRow& b = rows[1];
    const ResultRow& c = rows[2];
    CHECK(a.size() == 6 && b.size() == 6 && c.size() == 6);
    CHECK(a[0].str == "A" && b[0].str == "B" && c[0].str == "C");
    CHECK(a[1].i64 == 5 && b[1].i64 == 4 && c[1].i64 == 1);
    CHECK(decIs(a[2], 375, 2) && decIs(c[2], -5, 2));
    CHECK(b[2].isNull && b[2].type == GX_TYPE_DECIMAL);
    CHECK(a[3].type == GX_TYPE_F64 && a[3].f64 == 8.0 / 4.0);
    CHECK(b[3].type == GX_TYPE_F64 && b[3].isNull);
    CHECK(c[3].f64 == -1.5);
    // MIN compares under PAD SPACE and hands back the stored bytes
    CHECK(a[4].type == GX_TYPE_STRING && !a[4].isNull && a[4].str == "k ");
    CHECK(b[4].isNull && c[4].str == "m");
    // FIRSTROW: the group's first partial row wins, NULL or not
    CHECK(a[5].isNull && a[5].type == GX_TYPE_I64);
    CHECK(!b[5].isNull && b[5].i64 == 41 && c[5].i64 == 43);
  }
  // equal extremes under PAD SPACE: the first one stays
  {
    FinalSpec m;
    m.nGroup = 0;
    m.funcs = {GX_AGG_MIN, GX_AGG_MAX};
    m.fracs = {0, 0};
    m.argIsF64 = {0, 0};
    std::vector<std::vector<HostCol>> ch(1);
    ch[0] = {hostCol(GX_TYPE_STRING, {S("m "), S("m"), S("m  ")}),
             hostCol(GX_TYPE_STRING, {S("m "), S("m"), S("m  ")})};
    CHECK(mergeFinal(ch, m, &rows, &err) == GX_OK);
    CHECK(rows.size() == 1 && rows[0][0].str == "m " && rows[0][1].str == "m ");
  }
  // no chunks, no group-by: the scalar default row
  spec.nGroup = 0;
  CHECK(mergeFinal({}, spec, &rows, &err) == GX_OK);
  CHECK(rows.size() == 1 && rows[0].size() == 5);
  if (rows.size() == 1 && rows[0].size() == 5) {
    const ResultRow& r = rows[0];
    CHECK(r[0].type == GX_TYPE_I64 && !r[0].isNull && r[0].i64 == 0);
    CHECK(r[1].type == GX_TYPE_DECIMAL && r[1].isNull);
    CHECK(r[2].type == GX_TYPE_F64 && r[2].isNull);
    CHECK(r[3].isNull && r[4].isNull);
  }
  // with a group-by, no input is no output
  spec.nGroup = 1;
  CHECK(mergeFinal({}, spec, &rows, &err) == GX_OK && rows.empty());
}

// readCell on its own: every type, NULL and not
static void checkReadCell() {
  HostCol s = hostCol(GX_TYPE_STRING, {S("ab "), N(GX_TYPE_STRING), S("")});
  CHECK(readCell(s, 0).str == "ab " && readCell(s, 1).isNull);
  CHECK(!readCell(s, 2).isNull && readCell(s, 2).str.empty());
  HostCol d = hostCol(GX_TYPE_DECIMAL, {N(GX_TYPE_DECIMAL), D(-12345, 3)});
  CHECK(readCell(d, 0).isNull && decIs(readCell(d, 1), -12345, 3));
  HostCol f = hostCol(GX_TYPE_F64, {F(2.5)});
  CHECK(readCell(f, 0).type == GX_TYPE_F64 && readCell(f, 0).f64 == 2.5);
  HostCol t = hostCol(GX_TYPE_TIME, {T(0xABCDEF12345ULL)});
  CHECK(readCell(t, 0).type == GX_TYPE_TIME &&
        readCell(t, 0).u64 == 0xABCDEF12345ULL);
}

int main() {
  checkCompares();
  checkFinalizer();
  checkDistinct();
  checkHaving();
  checkSort();
  checkEmit();
  checkReadCell();
  checkMergeFinal();
  if (failures) {
    fprintf(stderr, "result_stage_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("result_stage_check OK\n");
  return 0;
}
