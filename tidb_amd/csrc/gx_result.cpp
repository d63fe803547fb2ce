// tidb_amd/csrc/gx_result.cpp — host result stage (see gx_result.h).
#include "gx_result.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <set>

namespace gxp {

MyDecimal decFromUnits(__int128 u, int scale) {
  MyDecimal d;
  const bool neg = u < 0;
  unsigned __int128 a = neg ? -(unsigned __int128)u : (unsigned __int128)u;
  // scale may exceed one decimal word (e.g. division results at 18): 10^scale
  // in 128 bits. Frac words hold 9 digits each, left-aligned (mydecimal.go
  // word layout): pad the trailing partial word to a word multiple.
  const int fw = (scale + 8) / 9;
  unsigned __int128 pscale = 1, pad = 1;
  for (int s = 0; s < scale; s++) pscale *= 10;
  for (int s = scale; s < fw * 9; s++) pad *= 10;
  unsigned __int128 ip = a / pscale, fr = a % pscale * pad;
  int32_t words[6];  // integer words, least significant first
  int nw = 0;
  do {
    words[nw++] = (int32_t)(ip % kWordBase);
    ip /= kWordBase;
  } while (ip > 0);
  // full words below the head, plus the head's own digits (zero counts one)
  int digitsInt = (nw - 1) * 9 + 1;
  for (int32_t head = words[nw - 1]; head >= 10; head /= 10) digitsInt++;
  d.digitsInt = (int8_t)digitsInt;
  d.digitsFrac = d.resultFrac = (int8_t)scale;
  d.negative = neg && a != 0;
  // wordBuf: integer words most significant first, then the frac words
  for (int i = 0; i < nw; i++) d.wordBuf[i] = words[nw - 1 - i];
  for (int i = fw - 1; i >= 0; i--) {
    d.wordBuf[nw + i] = (int32_t)(fr % kWordBase);
    fr /= kWordBase;
  }
  return d;
}

// ---------------- compares ----------------

template <class T>
static int cmp3(const T& x, const T& y) {
  return x < y ? -1 : (y < x ? 1 : 0);
}

static void trimPadSpace(std::string* s) {
  while (!s->empty() && s->back() == ' ') s->pop_back();
}

// NULL first; `order` selects the ORDER rules for TIME and strings
static int cmpCells(const OutRowVal& a, const OutRowVal& b, bool order) {
  if (a.isNull || b.isNull) return (int)b.isNull - (int)a.isNull;
  switch (a.type) {
    case GX_TYPE_DECIMAL:
      return a.dec.Compare(b.dec);
    case GX_TYPE_TIME: {
      uint64_t mask = order ? ~0xFULL : ~0ULL;
      return cmp3(a.u64 & mask, b.u64 & mask);
    }
    case GX_TYPE_STRING: {
      if (!order) return cmp3(a.str, b.str);
      std::string x = a.str, y = b.str;
      trimPadSpace(&x);
      trimPadSpace(&y);
      return cmp3(x, y);
    }
    case GX_TYPE_F64:
      return cmp3(a.f64, b.f64);
    default:
      return cmp3(a.i64, b.i64);
  }
}

int cmpOrder(const OutRowVal& a, const OutRowVal& b) {
  return cmpCells(a, b, true);
}

int cmpIdentity(const OutRowVal& a, const OutRowVal& b) {
  return cmpCells(a, b, false);
}

// ---------------- SUM / AVG finalize ----------------

static bool isSumFunc(int func) {
  return func == GX_AGG_SUM || func == GX_AGG_SUM_DISTINCT;
}

bool finalizeDecimalAgg(int func, const MyDecimal& sum, int64_t cnt, int frac,
                        OutRowVal* out) {
  out->type = GX_TYPE_DECIMAL;
  if (cnt == 0) {
    out->isNull = true;
    return true;
  }
  out->dec = sum;
  if (!isSumFunc(func)) {
    MyDecimal den;
    den.FromInt(cnt);
    int32_t ec = DecimalDiv(&sum, &den, &out->dec, kDivFracIncr);
    if (ec != E_OK && ec != E_TRUNCATED) return false;
  }
  out->dec.Round(&out->dec, frac, ModeHalfUp);
  return true;
}

void finalizeF64Agg(int func, double sum, int64_t cnt, OutRowVal* out) {
  out->type = GX_TYPE_F64;
  if (cnt == 0) out->isNull = true;
  else out->f64 = isSumFunc(func) ? sum : sum / (double)cnt;
}

// ---------------- DISTINCT fold ----------------

namespace {

struct TupleLess {
  bool operator()(const ResultRow& a, const ResultRow& b) const {
    for (size_t k = 0; k < a.size() && k < b.size(); k++) {
      int c = cmpIdentity(a[k], b[k]);
      if (c) return c < 0;
    }
    return a.size() < b.size();
  }
};

struct DistinctAcc {
  std::set<ResultRow, TupleLess> seen;
  int64_t cnt = 0;
  MyDecimal sum;
  DistinctAcc() { sum.FromInt(0); }
};
using DistinctAccs = std::vector<DistinctAcc>;  // one per aggregate

}  // namespace

int32_t foldDistinct(std::vector<ResultRow>* rows, const DistinctSpec& spec,
                     std::string* err) {
  // Inner rows are unique (keys, arg tuple) combinations; a single arg's
  // values can still repeat across rows (other args differ), so each agg
  // dedups ITS arg columns with a per-group set.
  const int nk = spec.nKeys;
  const size_t nA = spec.funcs.size();
  std::map<ResultRow, DistinctAccs, TupleLess> groups;  // by key cells
  std::vector<std::pair<const ResultRow, DistinctAccs>*> order;  // first seen
  for (const ResultRow& r : *rows) {
    auto [it, fresh] =
        groups.try_emplace(ResultRow(r.begin(), r.begin() + nk), nA);
    if (fresh) order.push_back(&*it);
    DistinctAccs& accs = it->second;
    for (size_t a = 0; a < nA; a++) {
      ResultRow tup;
      bool anyNull = false;
      for (int sl : spec.argSlot[a]) {
        const OutRowVal& v = r[nk + sl];
        anyNull |= v.isNull;
        tup.push_back(v);
      }
      if (anyNull) continue;  // NULL (any element) never counts distinct
      DistinctAcc& acc = accs[a];
      if (!acc.seen.insert(tup).second) continue;
      acc.cnt++;
      if (tup[0].type == GX_TYPE_DECIMAL &&
          spec.funcs[a] != GX_AGG_COUNT_DISTINCT) {
        MyDecimal tmp;
        int32_t ec = DecimalAdd(&acc.sum, &tup[0].dec, &tmp);
        if (ec != E_OK && ec != E_TRUNCATED) {
          *err = "distinct sum overflow";
          return GX_ERR_INTERNAL;
        }
        acc.sum = tmp;
      }
    }
  }
  if (nk == 0 && order.empty())  // scalar default row over zero rows
    order.push_back(&*groups.try_emplace(ResultRow(), nA).first);
  std::vector<ResultRow> folded;
  folded.reserve(order.size());
  for (const auto* g : order) {
    ResultRow row = g->first;
    for (size_t a = 0; a < nA; a++) {
      const DistinctAcc& acc = g->second[a];
      OutRowVal v;
      if (spec.funcs[a] == GX_AGG_COUNT_DISTINCT) {
        v.type = GX_TYPE_I64;
        v.i64 = acc.cnt;
      } else if (!finalizeDecimalAgg(spec.funcs[a], acc.sum, acc.cnt,
                                     spec.fracs[a], &v)) {
        *err = "distinct avg division failed";
        return GX_ERR_INTERNAL;
      }
      row.push_back(std::move(v));
    }
    folded.push_back(std::move(row));
  }
  *rows = std::move(folded);
  return GX_OK;
}

// ---------------- HAVING ----------------

// *typeOk goes false when the value and the constant do not pair
static bool leafPass(const HavingLeaf& l, const ResultRow& row, bool* typeOk) {
  if (l.col < 0 || l.col >= (int)row.size()) return *typeOk = false;
  const OutRowVal& v = row[l.col];
  if (l.isNullTest) return v.isNull == l.wantNull;
  if (v.isNull) return false;  // NULL rejects
  bool eqOnly = l.cmp == GX_F_EQ || l.cmp == GX_F_NE;
  bool pairs = v.type == l.cst.type &&
               (v.type == GX_TYPE_DECIMAL || v.type == GX_TYPE_I64 ||
                v.type == GX_TYPE_TIME ||
                (v.type == GX_TYPE_STRING && eqOnly));
  if (!pairs) return *typeOk = false;
  int c = cmpOrder(v, l.cst);
  switch (l.cmp) {
    case GX_F_LT: return c < 0;
    case GX_F_LE: return c <= 0;
    case GX_F_GT: return c > 0;
    case GX_F_GE: return c >= 0;
    case GX_F_EQ: return c == 0;
    default: return c != 0;
  }
}

bool havingPass(const ResultRow& row, const std::vector<HavingCond>& conds,
                bool* typeOk) {
  for (const HavingCond& cond : conds) {
    bool any = false;
    for (size_t i = 0; i < cond.size() && !any; i++)
      any = leafPass(cond[i], row, typeOk);
    if (!any) return false;
  }
  return true;
}

// ---------------- ORDER BY / LIMIT ----------------

void sortAndSlice(std::vector<ResultRow>* rows,
                  const std::vector<std::pair<int, bool>>& keys,
                  int64_t offset, int64_t limit) {
  std::stable_sort(rows->begin(), rows->end(),
                   [&](const ResultRow& a, const ResultRow& b) {
                     for (auto& [col, desc] : keys) {
                       int c = cmpOrder(a[col], b[col]);
                       if (desc) c = -c;
                       if (c != 0) return c < 0;
                     }
                     return false;
                   });
  size_t beginI = std::min<size_t>((size_t)offset, rows->size());
  size_t endI = limit < 0 ? rows->size()
                          : std::min<size_t>(beginI + (size_t)limit,
                                             rows->size());
  rows->erase(rows->begin() + endI, rows->end());
  rows->erase(rows->begin(), rows->begin() + beginI);
}

// ---------------- result marshalling ----------------

int32_t emitRows(const std::vector<ResultRow>& rows, size_t* pos,
                 gx_chunk* out, int32_t* rowsOut, std::string* err) {
  size_t n = std::min<size_t>(rows.size() - *pos, 1024);
  if (n == 0) {
    *rowsOut = 0;
    return GX_OK;
  }
  for (int c = 0; c < out->n_cols; c++) {
    if (out->cols[c].null_bitmap)
      std::memset(out->cols[c].null_bitmap, 0, ((int)n + 7) / 8);
    if (out->cols[c].offsets) out->cols[c].offsets[0] = 0;
  }
  for (size_t i = 0; i < n; i++) {
    const ResultRow& row = rows[*pos + i];
    if ((int)row.size() != out->n_cols) {
      *err = "output chunk column count mismatch";
      return GX_ERR_INVALID;
    }
    for (int c = 0; c < out->n_cols; c++) {
      const OutRowVal& v = row[c];
      gx_col* g = &out->cols[c];
      // a NULL string is an empty slice, a NULL fixed-width cell zero-filled
      const bool isStr = g->elem_size == -1 || v.type == GX_TYPE_STRING;
      const int es = v.type == GX_TYPE_DECIMAL ? 40 : 8;
      const int64_t len = v.isNull ? 0 : (int64_t)v.str.size();
      const bool fits = isStr ? g->offsets[i] + len <= g->data_cap &&
                                    (int64_t)i + 1 <= g->offsets_cap - 1
                              : (int64_t)(i + 1) * es <= g->data_cap;
      if (!fits) {
        *err = "output buffer too small";
        return GX_ERR_INVALID;
      }
      uint8_t* data = (uint8_t*)g->data;
      if (isStr) {
        if (len) std::memcpy(data + g->offsets[i], v.str.data(), len);
        g->offsets[i + 1] = g->offsets[i] + len;
      } else if (v.isNull) {
        std::memset(data + i * es, 0, es);
      } else {
        const void* src = v.type == GX_TYPE_DECIMAL ? (const void*)&v.dec
                          : v.type == GX_TYPE_F64   ? (const void*)&v.f64
                                                    : (const void*)&v.i64;
        std::memcpy(data + i * es, src, es);
      }
      if (!v.isNull && g->null_bitmap) g->null_bitmap[i / 8] |= 1 << (i % 8);
    }
  }
  for (int c = 0; c < out->n_cols; c++) out->cols[c].length = (int)n;
  out->n_rows = (int)n;
  *pos += n;
  *rowsOut = (int)n;
  return GX_OK;
}

// ---------------- FINAL-mode host merge ----------------

// cell i of a bound chunk column, its bytes read as a `type` cell. Only the
// member(s) of that type are filled: an F64 cell leaves i64/u64 at 0, an
// I64/TIME cell leaves f64 at 0.
static OutRowVal readCellAs(const HostCol& hc, int i, int type) {
  OutRowVal v;
  v.type = hc.type;
  const uint8_t* data = hc.data.data();
  if (!((hc.nullBitmap[i / 8] >> (i % 8)) & 1)) {
    v.isNull = true;
  } else if (type == GX_TYPE_STRING) {
    v.str.assign((const char*)data + hc.offsets[i],
                 hc.offsets[i + 1] - hc.offsets[i]);
  } else if (type == GX_TYPE_DECIMAL) {
    std::memcpy(&v.dec, data + i * 40, 40);
  } else if (type == GX_TYPE_F64) {
    std::memcpy(&v.f64, data + i * 8, 8);
  } else {
    std::memcpy(&v.u64, data + i * 8, 8);
    v.i64 = (int64_t)v.u64;
  }
  return v;
}

OutRowVal readCell(const HostCol& hc, int i) {
  return readCellAs(hc, i, hc.type);
}

// A group column's cell. Strings group under PAD SPACE, so they come back
// trimmed. DECIMAL and F64 group columns keep the merge's historical read:
// the first 8 bytes at stride 8 as an integer.
static OutRowVal readGroupCell(const HostCol& hc, int i) {
  bool asInt = hc.type == GX_TYPE_DECIMAL || hc.type == GX_TYPE_F64;
  OutRowVal v = readCellAs(hc, i, asInt ? (int)GX_TYPE_I64 : hc.type);
  trimPadSpace(&v.str);
  return v;
}

static int64_t readI64(const HostCol& hc, int i) {
  int64_t c;
  std::memcpy(&c, hc.data.data() + i * 8, 8);
  return c;
}

namespace {

struct FinalGroup {
  ResultRow groupVals;
  std::vector<MyDecimal> dec;
  std::vector<int64_t> cnt;
  ResultRow val;  // min/max/firstrow merged value
  std::vector<uint8_t> has;
  std::vector<double> f64;  // f64 sum partials
  explicit FinalGroup(size_t nAggs)
      : dec(nAggs), cnt(nAggs, 0), val(nAggs), has(nAggs, 0), f64(nAggs, 0.0) {}
};

}  // namespace

// fold partial row i of one chunk into its group's state
static bool mergePartialRow(const std::vector<HostCol>& ch, int i,
                            const FinalSpec& spec, FinalGroup* st) {
  size_t col = spec.nGroup;
  for (size_t a = 0; a < spec.funcs.size(); a++) {
    int f = spec.funcs[a];
    if (f == GX_AGG_COUNT) {
      st->cnt[a] += readI64(ch[col], i);
      col += 1;
    } else if (f == GX_AGG_MIN || f == GX_AGG_MAX) {
      // extreme of per-shard extremes; NULL partials (all-NULL shard) are
      // skipped (func_max_min.go merge)
      OutRowVal v = readCell(ch[col], i);
      if (!v.isNull) {
        int c = st->has[a] ? cmpOrder(v, st->val[a]) : 0;
        if (!st->has[a] || (f == GX_AGG_MAX ? c > 0 : c < 0)) {
          st->val[a] = std::move(v);
          st->has[a] = 1;
        }
      }
      col += 1;
    } else if (f == GX_AGG_FIRSTROW) {
      // first partial row of the group in input order (its value may
      // legitimately be NULL: the group's first row had a NULL arg)
      if (!st->has[a]) {
        st->val[a] = readCell(ch[col], i);
        st->has[a] = 1;
      }
      col += 1;
    } else {  // SUM/AVG: (f64 | decimal) partial sum + count
      int64_t c = readI64(ch[col + 1], i);
      if (c > 0 && ch[col].type == GX_TYPE_F64) {
        double v;
        std::memcpy(&v, ch[col].data.data() + i * 8, 8);
        st->f64[a] += v;
        st->cnt[a] += c;
      } else if (c > 0) {
        MyDecimal v, tmp;
        std::memcpy(&v, ch[col].data.data() + i * 40, 40);
        int32_t ec = DecimalAdd(&st->dec[a], &v, &tmp);
        if (ec != E_OK && ec != E_TRUNCATED) return false;
        st->dec[a] = tmp;
        st->cnt[a] += c;
      }
      col += 2;
    }
  }
  return true;
}

int32_t mergeFinal(const std::vector<std::vector<HostCol>>& chunks,
                   const FinalSpec& spec, std::vector<ResultRow>* rows,
                   std::string* err) {
  const size_t nAggs = spec.funcs.size();
  std::map<std::string, size_t> index;
  std::vector<FinalGroup> groups;  // first-seen order
  for (auto& ch : chunks) {
    int n = ch.empty() ? 0 : ch[0].length;
    for (int i = 0; i < n; i++) {
      // group identity: type-tagged raw values
      std::string key;
      ResultRow gvals;
      for (size_t g = 0; g < spec.nGroup; g++) {
        OutRowVal v = readGroupCell(ch[g], i);
        if (v.isNull) {
          key.push_back('\0');
        } else if (v.type == GX_TYPE_STRING) {
          key.push_back('\1');
          uint32_t l = (uint32_t)v.str.size();
          key.append((const char*)&l, 4);
          key.append(v.str);
        } else {
          key.push_back('\2');
          key.append((const char*)&v.u64, 8);
        }
        gvals.push_back(std::move(v));
      }
      auto it = index.find(key);
      if (it == index.end()) {
        groups.emplace_back(nAggs);
        groups.back().groupVals = std::move(gvals);
        it = index.emplace(std::move(key), groups.size() - 1).first;
      }
      if (!mergePartialRow(ch, i, spec, &groups[it->second])) {
        *err = "merge add failed";
        return GX_ERR_INTERNAL;
      }
    }
  }
  // zero partial rows, no group-by => the scalar-agg default row
  // (count=0, sums/extremes NULL — HashAggExec's empty-input semantics)
  if (spec.nGroup == 0 && groups.empty()) groups.emplace_back(nAggs);
  rows->clear();
  for (FinalGroup& st : groups) {
    ResultRow row = std::move(st.groupVals);
    for (size_t a = 0; a < nAggs; a++) {
      int f = spec.funcs[a];
      OutRowVal v;
      if (f == GX_AGG_COUNT) {
        v.type = GX_TYPE_I64;
        v.i64 = st.cnt[a];
      } else if (f == GX_AGG_MIN || f == GX_AGG_MAX || f == GX_AGG_FIRSTROW) {
        if (st.has[a]) {
          v = std::move(st.val[a]);
        } else {
          v.isNull = true;
          v.type = GX_TYPE_DECIMAL;
        }
      } else if (spec.argIsF64[a]) {
        finalizeF64Agg(f, st.f64[a], st.cnt[a], &v);
      } else if (!finalizeDecimalAgg(f, st.dec[a], st.cnt[a], spec.fracs[a],
                                     &v)) {
        *err = "avg finalize failed";
        return GX_ERR_INTERNAL;
      }
      row.push_back(std::move(v));
    }
    rows->push_back(std::move(row));
  }
  return GX_OK;
}

}  // namespace gxp
