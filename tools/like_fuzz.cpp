// tools/like_fuzz.cpp — stand-alone host check of tidb_amd/csrc/gx_like.h.
//
// Runs fixed cases, then a seeded random sweep comparing the iterative
// likeMatch (the source the kernels run) against the recursive DoMatchBinary
// definition, and the compiler against its invariants with exact-size heap
// buffers so a sanitizer sees any out-of-bounds write. Host code only:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I tidb_amd/csrc tools/like_fuzz.cpp \
//       -o build/like_fuzz && build/like_fuzz
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gx_like.h"

using namespace gxp;

// recursive definition (DoMatchBinary restated)
static bool refMatch(const uint8_t* s, int slen, const uint8_t* ch,
                     const uint8_t* tp, int n) {
  int si = 0;
  for (int i = 0; i < n; i++) {
    if (tp[i] == LIKE_MATCH) {
      if (si >= slen || s[si] != ch[i]) return false;
      si++;
    } else if (tp[i] == LIKE_ONE) {
      if (si >= slen) return false;
      si++;
    } else {
      i++;
      if (i == n) return true;
      for (; si < slen; si++)
        if ((tp[i] == LIKE_MATCH && ch[i] == s[si]) || tp[i] == LIKE_ONE)
          if (refMatch(s + si, slen - si, ch + i, tp + i, n - i)) return true;
      return false;
    }
  }
  return si == slen;
}

static int failures = 0;

static void check(bool ok, const char* what, const std::string& p,
                  const std::string& s) {
  if (ok) return;
  failures++;
  std::fprintf(stderr, "FAIL %s: pattern='%s' string='%s'\n", what, p.c_str(),
               s.c_str());
}

// compile with an exact-size heap buffer of `cap` elements
static int compileExact(const std::string& p, int esc, int cap,
                        std::vector<uint8_t>* ch, std::vector<uint8_t>* tp) {
  uint8_t* c = new uint8_t[cap > 0 ? cap : 1];
  uint8_t* t = new uint8_t[cap > 0 ? cap : 1];
  int n = likeCompile((const uint8_t*)p.data(), (int)p.size(), esc, c, t, cap);
  if (n >= 0) {
    ch->assign(c, c + n);
    tp->assign(t, t + n);
  }
  delete[] c;
  delete[] t;
  return n;
}

static int matchBoth(const std::string& p, int esc, const std::string& s) {
  LikePat lp;
  int n = likeCompilePat((const uint8_t*)p.data(), (int)p.size(), esc, &lp);
  if (n < 0) return -1;
  std::vector<uint8_t> ch, tp;
  int n2 = compileExact(p, esc, kLikeMaxElems, &ch, &tp);
  check(n2 == n, "compile count", p, s);
  // exact-size copy of the string so a read past [st, en) is caught
  uint8_t* buf = new uint8_t[s.size() ? s.size() : 1];
  std::memcpy(buf, s.data(), s.size());
  bool it = likeMatch(lp.chars, lp.types, lp.n, (const uint8_t*)buf, (int64_t)0,
                      (int64_t)s.size());
  bool rf = refMatch(buf, (int)s.size(), ch.data(), tp.data(), n);
  delete[] buf;
  check(it == rf, "iterative != recursive", p, s);
  return it ? 1 : 0;
}

int main() {
  struct Fixed { const char* p; int esc; const char* s; int want; };
  static const Fixed fixed[] = {
      {"%", 92, "", 1}, {"", 92, "", 1}, {"", 92, "x", 0}, {"_", 92, "", 0},
      {"_", 92, "%", 1}, {"A", 92, "a", 0}, {"BUILD%", 92, "BUILDING", 1},
      {"%ING", 92, "BUILDING", 1}, {"%ING", 92, "BUILDINGS", 0},
      {"%special%requests%", 92, "special packages requests", 1},
      {"%special%requests%", 92, "requests special", 0},
      {"h_llo%", 92, "hello world", 1}, {"_%_", 92, "x", 0},
      {"_%_", 92, "xy", 1}, {"%%x", 92, "x", 1}, {"%abac", 92, "abababac", 1},
      {"a%a%a", 92, "aaa", 1}, {"a%a%a", 92, "aa", 0},
      {"100\\%", 92, "100%", 1}, {"100\\%", 92, "1000", 0},
      {"%\\_%", 92, "a_b", 1}, {"a\\\\b", 92, "a\\b", 1},
      {"a\\b", 92, "a\\b", 1}, {"trail", 92, "trail  ", 0},
      {"\\", 92, "\\", 1}, {"50|% off|_now", 124, "50% off_now", 1},
      {"%|%%", 124, "100%", 1}, {"%|%%", 124, "hello", 0},
      {"%a-rather-long-string-beyond-si%", 92,
       "a-rather-long-string-beyond-sixteen-bytes", 1},
  };
  for (const Fixed& f : fixed)
    check(matchBoth(f.p, f.esc, f.s) == f.want, "fixed case", f.p, f.s);

  // limits: 32 elements fit, 33 do not; small caps never write past cap
  {
    std::vector<uint8_t> ch, tp;
    check(compileExact(std::string(32, 'a'), 92, 32, &ch, &tp) == 32, "cap 32",
          "a*32", "");
    check(compileExact(std::string(33, 'a'), 92, 32, &ch, &tp) == -1, "cap 33",
          "a*33", "");
    check(compileExact("%_%_", 92, 2, &ch, &tp) == -1, "cap rewrite", "%_%_",
          "");
    check(compileExact("a", 256, 8, &ch, &tp) == -2, "escape range", "a", "");
    LikePat lp;
    check(likeCompilePat((const uint8_t*)"aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", 33,
                         92, &lp) == -1, "pat 33", "a*33", "");
  }

  // seeded sweep: alphabet ab%_\ , patterns <= 12 bytes, strings <= 14 bytes
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  auto rnd = [&]() {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
  };
  static const char alpha[] = {'a', 'b', '%', '_', '\\'};
  long nMatch = 0, nTotal = 0;
  for (int it = 0; it < 300000; it++) {
    std::string p, s;
    int pl = (int)(rnd() % 13), sl = (int)(rnd() % 15);
    for (int i = 0; i < pl; i++) p.push_back(alpha[rnd() % 5]);
    for (int i = 0; i < sl; i++) s.push_back(alpha[rnd() % 5]);
    int esc = (rnd() % 8) ? 92 : 'b';
    // compile invariants at every cap: count is cap-independent, -1 iff over
    std::vector<uint8_t> ch, tp, ch2, tp2;
    int n = compileExact(p, esc, 16, &ch, &tp);
    check(n >= 0 && n <= pl, "count bound", p, s);
    for (int i = 0; i + 1 < n; i++)
      check(!(tp[i] == LIKE_ANY && tp[i + 1] != LIKE_MATCH),
            "ANY must be followed by a literal", p, s);
    int cap = (int)(rnd() % 6);
    int n3 = compileExact(p, esc, cap, &ch2, &tp2);
    check(n3 == (n <= cap ? n : -1), "cap handling", p, s);
    int r = matchBoth(p, esc, s);
    nTotal++;
    nMatch += r == 1;
  }
  std::printf("like_fuzz: %ld pairs, %ld matches, %d failures\n", nTotal,
              nMatch, failures);
  return failures == 0 && nMatch > 0 && nMatch < nTotal ? 0 : 1;
}
