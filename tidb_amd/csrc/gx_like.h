// tidb_amd/csrc/gx_like.h — general LIKE: compiled pattern + matcher, shared
// by the host plan compiler, the AOT kernels and the hipRTC sources.
//
// Binary collation, byte semantics (stringutil.CompilePatternBinary /
// DoMatchBinary restated): the pattern compiles to <= kLikeMaxElems
// (char, type) elements; `_` consumes exactly one BYTE, `%` any run
// (including the empty one), everything else one equal byte. Matching is
// case-sensitive, consumes the whole string and trims nothing (LIKE has no
// PAD SPACE semantics).
#ifndef GX_LIKE_H
#define GX_LIKE_H

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define GX_LIKE_HD __host__ __device__
#else
#define GX_LIKE_HD
#endif

namespace gxp {

constexpr int kLikeMaxElems = 32;  // 2-bit types fill one u64; chars 32 B
enum LikeType : int32_t { LIKE_MATCH = 0, LIKE_ONE = 1, LIKE_ANY = 2 };

// compiled pattern as it travels in descriptors: chars[i] is the literal of
// element i (MATCH only), types holds element i's LikeType at bits [2i, 2i+2)
struct LikePat {
  uint8_t chars[kLikeMaxElems] = {0};
  uint64_t types = 0;
  int32_t n = 0;
  int32_t pad = 0;
};

GX_LIKE_HD inline int likeTypeAt(uint64_t types, int i) {
  return (int)((types >> (2 * i)) & 3);
}

// pattern compile (host): walks the bytes with a lastAny flag. `%%`
// collapses, `%_` reorders to `_%`, an escape followed by escape/_/% emits
// that byte as a literal, any other (or a trailing) escape is itself a
// literal. Returns the element count, -1 when it exceeds cap, -2 on an
// escape outside 0..255.
inline int32_t likeCompile(const uint8_t* pat, int32_t len, int32_t escape,
                           uint8_t* outChars, uint8_t* outTypes, int32_t cap) {
  if (escape < 0 || escape > 255 || len < 0) return -2;
  int32_t n = 0;
  bool lastAny = false;
  for (int32_t i = 0; i < len; i++) {
    uint8_t c = pat[i];
    uint8_t t;
    if (c == (uint8_t)escape) {
      lastAny = false;
      t = LIKE_MATCH;
      if (i < len - 1) {
        uint8_t nx = pat[i + 1];
        if (nx == (uint8_t)escape || nx == '_' || nx == '%') {
          c = nx;
          i++;
        }
      }
    } else if (c == '_') {
      if (lastAny) {  // %_ => _%
        if (n >= cap) return -1;
        outChars[n - 1] = '_';
        outTypes[n - 1] = LIKE_ONE;
        outChars[n] = '%';
        outTypes[n] = LIKE_ANY;
        n++;
        continue;
      }
      t = LIKE_ONE;
    } else if (c == '%') {
      if (lastAny) continue;
      t = LIKE_ANY;
      lastAny = true;
    } else {
      t = LIKE_MATCH;
      lastAny = false;
    }
    if (n >= cap) return -1;
    outChars[n] = c;
    outTypes[n] = t;
    n++;
  }
  return n;
}

// compile straight into the descriptor form; same return codes with
// cap = kLikeMaxElems
inline int32_t likeCompilePat(const uint8_t* pat, int32_t len, int32_t escape,
                              LikePat* out) {
  uint8_t ch[kLikeMaxElems], tp[kLikeMaxElems];
  int32_t n = likeCompile(pat, len, escape, ch, tp, kLikeMaxElems);
  if (n < 0) return n;
  *out = LikePat{};
  for (int32_t i = 0; i < n; i++) {
    out->chars[i] = tp[i] == LIKE_MATCH ? ch[i] : 0;
    out->types |= (uint64_t)tp[i] << (2 * i);
  }
  out->n = n;
  return n;
}

// iterative matcher over bytes p[st, en): two cursors plus the last ANY and
// the string position to resume from -- no recursion, no scratch. P is any
// byte-indexable pointer (address-space-1 loads on device, plain on host).
// Reads only p[si] with st <= si < en.
template <typename P>
GX_LIKE_HD inline bool likeMatch(const uint8_t* chars, uint64_t types, int n,
                                 P p, int64_t st, int64_t en) {
  int64_t si = st, resume = st;
  int pi = 0, star = -1;
  while (si < en) {
    int t = pi < n ? likeTypeAt(types, pi) : -1;
    if (t == LIKE_ONE || (t == LIKE_MATCH && chars[pi] == (uint8_t)p[si])) {
      si++;
      pi++;
    } else if (t == LIKE_ANY) {
      if (pi == n - 1) return true;  // trailing %: the rest matches
      star = pi++;
      resume = si;
    } else if (star >= 0) {
      pi = star + 1;
      si = ++resume;
    } else {
      return false;
    }
  }
  while (pi < n && likeTypeAt(types, pi) == LIKE_ANY) pi++;
  return pi == n;
}

}  // namespace gxp

#endif
