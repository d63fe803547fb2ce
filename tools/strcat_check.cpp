// tools/strcat_check.cpp — stand-alone host check of tidb_amd/csrc/gx_strcat.h.
//
// Runs fixed cases, then a seeded random sweep of the integer text, the
// window fold and the whole composed-string path (length pass, prefix sum,
// tile-by-tile byte mapping: the source the kernels run) against a
// straightforward std::string reference. Every buffer the header's code
// reads or writes is a heap block of exactly the needed size, so a sanitizer
// sees any out-of-bounds access. Host code only:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I tidb_amd/csrc tools/strcat_check.cpp \
//       -o build/strcat_check && build/strcat_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gx_strcat.h"

using namespace gxp;

static int failures = 0;

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
// random magnitude and sign, built in uint64_t (no signed overflow)
static int64_t rndI64() {
  uint64_t u = rnd() >> rndInt(0, 63);
  return (int64_t)(rndInt(0, 1) ? u : (uint64_t)0 - u);
}

// ---- integer text ----
static void checkI64(int64_t v) {
  std::string want = std::to_string((long long)v);
  int len = i64TextLen(v);
  if (len != (int)want.size()) {
    fail("i64TextLen", want);
    return;
  }
  uint8_t* buf = (uint8_t*)std::malloc(len);  // exact size
  for (int j = 0; j < len; j++) buf[j] = i64TextByte(v, len, j);
  if (std::memcmp(buf, want.data(), len) != 0) fail("i64TextByte", want);
  std::free(buf);
}

// ---- reference window (MySQL SUBSTR / TRIM on std::string) ----
static std::string refWindow(std::string s, const StrPiece& pc) {
  for (int w = 0; w < pc.nWin; w++) {
    long long pos = pc.winPos[w], L = pc.winLen[w];
    if (L == -1) {
      size_t a = s.find_first_not_of(' ');
      if (a == std::string::npos) { s.clear(); continue; }
      size_t b = s.find_last_not_of(' ');
      s = s.substr(a, b - a + 1);
      continue;
    }
    long long len = (long long)s.size();
    long long start = pos < 0 ? len + pos + 1 : pos;
    if (start < 1 || start > len || L <= 0) return "";
    s = s.substr((size_t)(start - 1), (size_t)L);
  }
  if (pc.caseOp == SCO_UPPER)
    for (char& c : s) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
  if (pc.caseOp == SCO_LOWER)
    for (char& c : s) if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}

// one input column on the heap, exact sizes
struct Col {
  bool isInt = false;
  int64_t n = 0;
  uint8_t* data = nullptr;    // string bytes
  int64_t* offsets = nullptr; // n + 1
  int64_t* ints = nullptr;    // n
  uint8_t* nulls = nullptr;   // (n + 7) / 8, 1 = NOT NULL; null = no NULLs
  std::vector<std::string> sv;  // reference copies
  std::vector<int64_t> iv;
  std::vector<bool> isNull;
  void release() {
    std::free(data); std::free(offsets); std::free(ints); std::free(nulls);
  }
};

static Col makeStrCol(const std::vector<std::string>& vals,
                      const std::vector<bool>& isNull, bool withBitmap) {
  Col c;
  c.n = (int64_t)vals.size();
  c.sv = vals;
  c.isNull = isNull;
  size_t total = 0;
  for (auto& s : vals) total += s.size();
  c.data = (uint8_t*)std::malloc(total ? total : 1);
  c.offsets = (int64_t*)std::malloc((vals.size() + 1) * 8);
  size_t at = 0;
  for (size_t i = 0; i < vals.size(); i++) {
    c.offsets[i] = (int64_t)at;
    std::memcpy(c.data + at, vals[i].data(), vals[i].size());
    at += vals[i].size();
  }
  c.offsets[vals.size()] = (int64_t)at;
  if (withBitmap) {
    size_t nb = (vals.size() + 7) / 8;
    c.nulls = (uint8_t*)std::calloc(nb ? nb : 1, 1);
    for (size_t i = 0; i < vals.size(); i++)
      if (!isNull[i]) c.nulls[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  return c;
}

static Col makeIntCol(const std::vector<int64_t>& vals,
                      const std::vector<bool>& isNull, bool withBitmap) {
  Col c;
  c.isInt = true;
  c.n = (int64_t)vals.size();
  c.iv = vals;
  c.isNull = isNull;
  c.ints = (int64_t*)std::malloc(vals.size() ? vals.size() * 8 : 1);
  for (size_t i = 0; i < vals.size(); i++) c.ints[i] = vals[i];
  if (withBitmap) {
    size_t nb = (vals.size() + 7) / 8;
    c.nulls = (uint8_t*)std::calloc(nb ? nb : 1, 1);
    for (size_t i = 0; i < vals.size(); i++)
      if (!isNull[i]) c.nulls[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  return c;
}

// reference: one output row as a std::string, row-wise append
static bool refRow(const StrCatProg& pg, const uint8_t* pool,
                   const std::vector<const Col*>& pieceCol, int64_t row,
                   std::string* out) {
  out->clear();
  bool any = false;
  std::string sep((const char*)pool + pg.sepOff, pg.sepLen);
  for (int p = 0; p < pg.nPieces; p++) {
    const StrPiece& pc = pg.piece[p];
    std::string part;
    bool nul = false;
    if (pc.kind == SPK_CONST) {
      part.assign((const char*)pool + pc.constOff, pc.constLen);
    } else {
      const Col& c = *pieceCol[p];
      nul = c.isNull[row];
      if (!nul)
        part = pc.kind == SPK_I64 ? std::to_string((long long)c.iv[row])
                                  : refWindow(c.sv[row], pc);
    }
    if (nul) {
      if (!pg.ws) return false;  // CONCAT: any NULL -> NULL
      continue;                  // CONCAT_WS: skipped with its separator
    }
    if (pg.ws && any) *out += sep;
    *out += part;
    any = true;
  }
  return true;
}

// run the header's passes over exact-size buffers and compare
static void runCase(const char* name, const StrCatProg& pg, const uint8_t* pool,
                    const std::vector<const Col*>& pieceCol, int64_t n) {
  StrCatHostSrc src;
  src.poolp = pool;
  for (int p = 0; p < pg.nPieces; p++) {
    if (pg.piece[p].kind == SPK_CONST) continue;
    const Col& c = *pieceCol[p];
    src.nullBitmap[p] = c.nulls;
    if (c.isInt) src.i64[p] = c.ints;
    else { src.data[p] = c.data; src.offsets[p] = c.offsets; }
  }
  int64_t* lens = (int64_t*)std::malloc(n ? n * 8 : 1);
  uint8_t* notNull = (uint8_t*)std::malloc(n ? n : 1);
  int64_t* off = (int64_t*)std::malloc((n + 1) * 8);
  if (!strCatHostLens(pg, src, n, lens, notNull)) fail(name, "row too long");
  off[0] = 0;
  for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + lens[i];
  uint8_t* out = (uint8_t*)std::malloc(off[n] ? off[n] : 1);
  strCatHostEmit(pg, src, n, off, out);
  for (int64_t r = 0; r < n; r++) {
    std::string want;
    bool nn = refRow(pg, pool, pieceCol, r, &want);
    if (nn != (notNull[r] != 0)) { fail(name, "null flag, row " + std::to_string(r)); continue; }
    if (!nn) {
      if (lens[r] != 0) fail(name, "NULL row with bytes");
      continue;
    }
    if ((int64_t)want.size() != lens[r] ||
        std::memcmp(out + off[r], want.data(), want.size()) != 0)
      fail(name, "row " + std::to_string(r) + " want '" + want.substr(0, 60) + "'");
  }
  std::free(lens); std::free(notNull); std::free(off); std::free(out);
}

static const char* kStrs[] = {"hello world", "", "A", "BUILDING", "mixed-Case-Str",
                              "a-rather-long-string-beyond-sixteen-bytes",
                              "trail  ", "  lead", "x", "   ", " a b "};

static std::vector<std::string> randStrs(int64_t n, std::vector<bool>* isNull,
                                         int nullPct, int64_t longRow) {
  std::vector<std::string> v(n);
  isNull->assign(n, false);
  for (int64_t i = 0; i < n; i++) {
    if (rndInt(0, 99) < nullPct) { (*isNull)[i] = true; continue; }
    v[i] = kStrs[rnd() % (sizeof kStrs / sizeof kStrs[0])];
  }
  if (longRow >= 0 && longRow < n) {
    (*isNull)[longRow] = false;
    v[longRow].assign(70000, 'q');
    for (size_t k = 0; k < v[longRow].size(); k += 7) v[longRow][k] = (char)('a' + k % 26);
  }
  return v;
}

static std::vector<int64_t> randInts(int64_t n, std::vector<bool>* isNull, int nullPct) {
  static const int64_t edge[] = {0, -1, 9, 10, -10, 1000000000000000000LL,
                                 INT64_MAX, INT64_MIN};
  std::vector<int64_t> v(n);
  isNull->assign(n, false);
  for (int64_t i = 0; i < n; i++) {
    if (rndInt(0, 99) < nullPct) { (*isNull)[i] = true; v[i] = (int64_t)rnd(); continue; }
    v[i] = rndInt(0, 2) == 0 ? edge[rnd() % 8] : rndI64();
  }
  return v;
}

static void randomProgram(StrCatProg* pg, uint8_t* pool, int* poolLen,
                          std::vector<const Col*>* pieceCol, const Col* s0,
                          const Col* s1, const Col* ic) {
  *pg = StrCatProg{};
  *poolLen = 0;
  auto addConst = [&](uint16_t* off, uint16_t* len) {
    int l = rndInt(0, 5);
    *off = (uint16_t)*poolLen;
    *len = (uint16_t)l;
    for (int i = 0; i < l; i++) pool[(*poolLen)++] = (uint8_t)("-,#x /"[rnd() % 6]);
  };
  pg->ws = (uint8_t)rndInt(0, 1);
  if (pg->ws) addConst(&pg->sepOff, &pg->sepLen);
  pg->nPieces = (uint8_t)rndInt(1, kStrCatMaxPieces);
  pieceCol->assign(pg->nPieces, nullptr);
  for (int p = 0; p < pg->nPieces; p++) {
    StrPiece& pc = pg->piece[p];
    int k = rndInt(0, 3);
    if (k == 0) {
      pc.kind = SPK_CONST;
      addConst(&pc.constOff, &pc.constLen);
    } else if (k == 1) {
      pc.kind = SPK_I64;
      pc.col = 2;
      (*pieceCol)[p] = ic;
    } else {
      pc.kind = SPK_WINDOW;
      pc.col = (int16_t)rndInt(0, 1);
      (*pieceCol)[p] = pc.col == 0 ? s0 : s1;
      pc.caseOp = (uint8_t)rndInt(0, 2);
      pc.nWin = (uint8_t)rndInt(0, kStrCatMaxWin);
      for (int w = 0; w < pc.nWin; w++) {
        if (rndInt(0, 3) == 0) { pc.winPos[w] = 0; pc.winLen[w] = -1; continue; }
        pc.winPos[w] = rndInt(-12, 12);
        int l = rndInt(-1, 14);
        pc.winLen[w] = l == -1 ? 0x7FFFFFFF : l;  // -1 is the TRIM marker
      }
    }
  }
}

int main() {
  // integer text: every power of ten and its neighbour, the extremes
  checkI64(0);
  checkI64(INT64_MAX);
  checkI64(INT64_MIN);
  int64_t p = 1;
  for (int k = 0; k <= 18; k++) {
    checkI64(p); checkI64(-p); checkI64(p - 1); checkI64(-(p - 1));
    checkI64(p + 1); checkI64(-(p + 1));
    if (k < 18) p *= 10;
  }
  for (int i = 0; i < 200000; i++)
    checkI64(rndI64());
  if (strWinSaturate(1LL << 40) != 0x7FFFFFFF || strWinSaturate(-(1LL << 40)) != -0x7FFFFFFF ||
      strWinSaturate(-1) != -1 || strWinSaturate(7) != 7)
    fail("strWinSaturate", "");

  // row finder: zero-length rows are never returned
  {
    int64_t* off = (int64_t*)std::malloc(6 * 8);
    int64_t v[6] = {10, 10, 13, 13, 13, 14};
    std::memcpy(off, v, sizeof v);
    if (strCatFindRow(off, 5, 10) != 1 || strCatFindRow(off, 5, 12) != 1 ||
        strCatFindRow(off, 5, 13) != 4)
      fail("strCatFindRow", "fixed");
    std::free(off);
  }

  // composed strings: tile edges, a 70 000-byte row, all-NULL and all-empty
  // columns, random programs
  const int64_t sizes[] = {0, 1, 255, 256, 257, 600};
  for (int iter = 0; iter < 240; iter++) {
    int64_t n = sizes[iter % 6];
    std::vector<bool> n0, n1, ni;
    int mode = iter % 5;
    int64_t longRow = (iter % 7 == 3 && n > 1) ? n / 2 : -1;
    auto v0 = randStrs(n, &n0, mode == 1 ? 100 : 15, longRow);
    auto v1 = randStrs(n, &n1, 15, -1);
    if (mode == 2) {  // every string empty
      for (auto& s : v0) s.clear();
      for (auto& s : v1) s.clear();
      n0.assign(n, false);
      n1.assign(n, false);
    }
    auto vi = randInts(n, &ni, mode == 3 ? 100 : 15);
    Col s0 = makeStrCol(v0, n0, true);
    Col s1 = makeStrCol(v1, n1, iter % 2 == 0);
    if (iter % 2 != 0) { n1.assign(n, false); s1.isNull = n1; }
    Col ic = makeIntCol(vi, ni, true);
    StrCatProg pg;
    uint8_t* pool = (uint8_t*)std::malloc(kStrCatPoolBytes);
    int poolLen = 0;
    std::vector<const Col*> pieceCol;
    randomProgram(&pg, pool, &poolLen, &pieceCol, &s0, &s1, &ic);
    if (mode == 2) {  // CONCAT(s0, s1) over empty strings: 0 bytes, n rows
      pg = StrCatProg{};
      pg.nPieces = 2;
      pg.piece[0].kind = pg.piece[1].kind = SPK_WINDOW;
      pg.piece[0].col = 0;
      pg.piece[1].col = 1;
      pieceCol = {&s0, &s1};
    }
    // the pool as an exact-size block
    uint8_t* exactPool = (uint8_t*)std::malloc(poolLen ? poolLen : 1);
    std::memcpy(exactPool, pool, poolLen);
    std::free(pool);
    runCase("sweep", pg, exactPool, pieceCol, n);
    std::free(exactPool);
    s0.release(); s1.release(); ic.release();
  }
  if (failures) {
    std::fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  std::printf("strcat_check OK\n");
  return 0;
}
