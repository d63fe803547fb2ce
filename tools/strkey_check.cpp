// tools/strkey_check.cpp — stand-alone host check of tidb_amd/csrc/gx_strkey.h.
//
// Fixed cases, then a seeded random sweep (lengths 0..40, an alphabet
// weighted toward 0x00, 0x20, 0x7F, 0x80, 0xFF, shared prefixes) of
//   1. the window keys: the sign of the lexicographic compare of
//      W(a,0), W(a,1), ... and W(b,0), W(b,1), ... equals the sign of the
//      reference compare (utf8mb4_bin PAD SPACE, BinCollatorKey restated:
//      trim trailing spaces, then std::string::compare);
//   2. the whole refinement as the engine's buildStringRank runs it, with
//      std::stable_sort in place of the two radix passes: the ranks are
//      consistent with that compare (less iff less, equal iff equal), and the
//      round count stays inside strKeyMaxRounds.
// Every string lives in a heap block of exactly its length, and the windows
// read a block of exactly the effective length, so a sanitizer sees any
// byte read at or past the end. Host code only:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I tidb_amd/csrc tools/strkey_check.cpp \
//       -o build/strkey_check && build/strkey_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "gx_strkey.h"

using namespace gxp;

static int failures = 0;

static std::string show(const std::string& s) {
  std::string o;
  char b[8];
  for (unsigned char c : s) {
    std::snprintf(b, sizeof b, "%02x", c);
    o += b;
  }
  return "[" + o + "]";
}

static void fail(const char* what, const std::string& detail) {
  failures++;
  if (failures <= 20)
    std::fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

// xorshift64*: the sweep is seeded and repeatable
static uint64_t rngState = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
  rngState ^= rngState >> 12;
  rngState ^= rngState << 25;
  rngState ^= rngState >> 27;
  return rngState * 0x2545F4914F6CDD1DULL;
}
static int rndInt(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

static int sign(int v) { return v < 0 ? -1 : (v > 0 ? 1 : 0); }

// ---- reference: trim, then compare as unsigned bytes, shorter first
static std::string trimmed(const std::string& s) {
  size_t n = s.size();
  while (n > 0 && s[n - 1] == ' ') n--;
  return s.substr(0, n);
}
static int refCompare(const std::string& a, const std::string& b) {
  return sign(trimmed(a).compare(trimmed(b)));
}

// ---- one string on the heap: the row's bytes at exactly their length, and
// the effective string at exactly its length (null for length 0)
struct Row {
  uint8_t* full = nullptr;
  uint8_t* eff = nullptr;
  uint32_t elen = 0;
  bool isNull = false;
};

struct Bytes {
  const uint8_t* p;
  uint8_t operator()(int64_t i) const { return p[i]; }
};

static Row makeRow(const std::string& s, bool isNull) {
  Row r;
  r.isNull = isNull;
  if (isNull) return r;  // the bytes under a NULL are never read
  if (!s.empty()) {
    r.full = (uint8_t*)std::malloc(s.size());
    std::memcpy(r.full, s.data(), s.size());
  }
  r.elen = (uint32_t)strKeyTrimLen(Bytes{r.full}, 0, (int64_t)s.size());
  if (r.elen) {
    r.eff = (uint8_t*)std::malloc(r.elen);
    std::memcpy(r.eff, r.full, r.elen);
  }
  return r;
}

static void freeRow(Row& r) {
  std::free(r.full);
  std::free(r.eff);
}

static uint64_t window(const Row& r, uint32_t round) {
  return strKeyWindow(Bytes{r.eff}, 0, r.elen, round);
}

// ---- 1. window sequences against the reference
static void checkPair(const std::string& a, const std::string& b) {
  Row ra = makeRow(a, false), rb = makeRow(b, false);
  if (ra.elen != trimmed(a).size()) fail("strKeyTrimLen", show(a));
  uint32_t rounds = strKeyMaxRounds(std::max(ra.elen, rb.elen));
  int got = 0;
  for (uint32_t r = 0; r < rounds && got == 0; r++) {
    uint64_t wa = window(ra, r), wb = window(rb, r);
    got = wa < wb ? -1 : (wa > wb ? 1 : 0);
    // a finished row ties only with an equal one
    if (got == 0 && strKeyCount(wa) < kStrKeyWin && refCompare(a, b) != 0)
      fail("finished rows tie but differ", show(a) + " " + show(b));
  }
  // past the bound every window is zero
  if (window(ra, rounds) != 0 || window(rb, rounds) != 0)
    fail("window past the round bound", show(a) + " " + show(b));
  if (got != refCompare(a, b))
    fail("window order", show(a) + " vs " + show(b));
  freeRow(ra);
  freeRow(rb);
}

// ---- 2. the refinement (buildStringRank, host model)
static std::vector<uint32_t> modelRanks(const std::vector<Row>& rows,
                                        uint32_t* roundsOut) {
  const int64_t n = (int64_t)rows.size();
  std::vector<uint32_t> rank(n, 0), perm(n, 0), head(n, 0);
  uint32_t maxElen = 0;
  for (const Row& r : rows) maxElen = std::max(maxElen, r.elen);
  const uint32_t maxRounds = strKeyMaxRounds(maxElen);
  std::vector<uint32_t> act(n);
  std::iota(act.begin(), act.end(), 0u);
  bool identity = true;  // round 0: position i holds row i
  uint32_t round = 0;
  while (!act.empty()) {
    if (round >= maxRounds) {
      fail("round bound", "refinement ran past strKeyMaxRounds");
      break;
    }
    const int64_t m = (int64_t)act.size();
    std::vector<uint64_t> w(m), wSorted(m);
    std::vector<uint32_t> rowAct(m), seg(m), order(m);
    uint32_t run = 0;
    for (int64_t i = 0; i < m; i++) {
      uint32_t row = identity ? (uint32_t)i : perm[act[i]];
      uint32_t hf = identity ? (i == 0) : head[act[i]];
      w[i] = window(rows[row], round);
      rowAct[i] = row;
      run += hf;
      seg[i] = run;  // inclusive sum of the head flags: 1..nSeg
    }
    if (seg[0] != 1) fail("segment", "an active range does not start at a head");
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return w[a] < w[b]; });
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return seg[a] < seg[b]; });
    for (int64_t j = 0; j < m; j++) {
      // rows return to their own tied range
      if (seg[order[j]] != seg[j]) fail("segment", "a row left its range");
      wSorted[j] = w[order[j]];
      perm[act[j]] = rowAct[order[j]];
    }
    std::vector<uint32_t> next;
    for (int64_t j = 0; j < m; j++) {
      if (strKeyIsHead(seg, wSorted, j)) head[act[j]] = 1;
      if (strKeyStaysActive(seg, wSorted, j, m)) next.push_back(act[j]);
    }
    act.swap(next);
    identity = false;
    round++;
  }
  uint32_t scan = 0;
  for (int64_t pos = 0; pos < n; pos++) {
    scan += head[pos];
    rank[perm[pos]] = scan - 1;
  }
  *roundsOut = round;
  return rank;
}

static void checkRanks(const std::vector<std::string>& strs,
                       const std::vector<bool>& nulls, const char* what) {
  std::vector<Row> rows;
  std::vector<std::string> key;  // what a row compares as: NULL as ""
  for (size_t i = 0; i < strs.size(); i++) {
    rows.push_back(makeRow(strs[i], nulls[i]));
    key.push_back(nulls[i] ? std::string() : strs[i]);
  }
  uint32_t rounds = 0;
  std::vector<uint32_t> rank = modelRanks(rows, &rounds);
  const size_t n = strs.size();
  // every adjacent pair in rank order, plus random pairs
  std::vector<uint32_t> byRank(n);
  std::iota(byRank.begin(), byRank.end(), 0u);
  std::stable_sort(byRank.begin(), byRank.end(),
                   [&](uint32_t a, uint32_t b) { return rank[a] < rank[b]; });
  auto pair = [&](uint32_t a, uint32_t b) {
    int want = refCompare(key[a], key[b]);
    int got = rank[a] < rank[b] ? -1 : (rank[a] > rank[b] ? 1 : 0);
    if (want != got) fail(what, show(key[a]) + " vs " + show(key[b]));
  };
  for (size_t i = 1; i < n; i++) {
    pair(byRank[i - 1], byRank[i]);
    // dense: a step of at most one
    if (rank[byRank[i]] - rank[byRank[i - 1]] > 1) fail(what, "rank gap");
  }
  if (n && rank[byRank[0]] != 0) fail(what, "ranks do not start at 0");
  for (size_t i = 0; i < 4 * n; i++)
    pair((uint32_t)rndInt(0, (int)n - 1), (uint32_t)rndInt(0, (int)n - 1));
  for (Row& r : rows) freeRow(r);
}

// ---- random strings
static const uint8_t kHeavy[] = {0x00, 0x20, 0x7F, 0x80, 0xFF, 'a', 'b'};

static std::string rndString(const std::vector<std::string>& pool) {
  std::string s;
  if (!pool.empty() && rndInt(0, 2) != 0) {  // a prefix of an earlier string
    const std::string& p = pool[rndInt(0, (int)pool.size() - 1)];
    s = p.substr(0, (size_t)rndInt(0, (int)p.size()));
  }
  int len = rndInt(0, 40);
  while ((int)s.size() < len)
    s.push_back((char)(rndInt(0, 9) < 8 ? kHeavy[rndInt(0, 6)]
                                        : (uint8_t)rndInt(0, 255)));
  if ((int)s.size() > len) s.resize(len);
  if (rndInt(0, 3) == 0) s.append((size_t)rndInt(1, 9), ' ');
  if (s.size() > 40) s.resize(40);
  return s;
}

int main() {
  const std::string z("\0", 1);
  std::vector<std::string> fixed = {
      "", " ", z, "ab", "ab ", "ab  ", "ab" + z, "ab" + z + z, "ab" + z + "a",
      "ab c", "abcdefg", "abcdefg ", "abcdefg" + z, "abcdefgh", "abcdef",
      "abcdefghijklmn", "abcdefghijklm", "abcdefghijklmn" + z,
      "abcdefghijklmno", std::string(7, ' '), std::string(8, ' '),
      "\x7f", "\x80", "\xff", "a\x7f", "a\x80", "a\xff", "abcdefg\x80",
      "abcdefg\x7f", std::string(40, 'x'), std::string(40, 'x') + "",
      std::string(39, 'x') + "y", std::string(30, 'p') + "a",
      std::string(30, 'p') + "b", std::string(30, 'p'),
      std::string(14, 'q') + " ", std::string(14, 'q') + " q"};
  for (const std::string& a : fixed)
    for (const std::string& b : fixed) checkPair(a, b);
  {
    std::vector<bool> nulls(fixed.size(), false);
    checkRanks(fixed, nulls, "fixed ranks");
    std::vector<std::string> one = {"abc"}, none;
    checkRanks(one, std::vector<bool>(1, false), "one row");
    checkRanks(none, std::vector<bool>(), "no rows");
    std::vector<std::string> eq(100, std::string(40, 'e'));
    std::vector<bool> n4(100, false);
    checkRanks(eq, n4, "all equal");
    for (size_t i = 0; i < n4.size(); i += 4) n4[i] = true;
    checkRanks(eq, n4, "all equal, nullable");
  }
  for (int iter = 0; iter < 400; iter++) {
    std::vector<std::string> strs;
    std::vector<bool> nulls;
    int n = rndInt(1, 120);
    for (int i = 0; i < n; i++) {
      strs.push_back(rndString(strs));
      nulls.push_back(rndInt(0, 9) == 0);
    }
    for (int i = 0; i < 2 * n; i++)
      checkPair(strs[rndInt(0, n - 1)], strs[rndInt(0, n - 1)]);
    checkRanks(strs, nulls, "random ranks");
  }
  // f64 key: order of the keys == order of the doubles, -0.0 ties with 0.0
  {
    const double vals[] = {-1e308, -1.5, -4.9e-324, -0.0, 0.0, 4.9e-324,
                           1.0, 1.0000000000000002, 1e308};
    const int nv = (int)(sizeof vals / sizeof vals[0]);
    for (int i = 0; i < nv; i++)
      for (int j = 0; j < nv; j++) {
        uint64_t bi, bj;
        std::memcpy(&bi, &vals[i], 8);
        std::memcpy(&bj, &vals[j], 8);
        uint64_t ki = f64OrderKey(bi), kj = f64OrderKey(bj);
        int want = vals[i] < vals[j] ? -1 : (vals[i] > vals[j] ? 1 : 0);
        int got = ki < kj ? -1 : (ki > kj ? 1 : 0);
        if (want != got) fail("f64OrderKey", std::to_string(vals[i]));
      }
  }
  if (failures) {
    std::fprintf(stderr, "strkey_check: %d failures\n", failures);
    return 1;
  }
  std::printf("strkey_check: OK\n");
  return 0;
}
