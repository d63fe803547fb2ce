// tidb_amd/csrc/gx_strkey.h — order keys of variable-length strings for the
// device sort: the effective length, the 7-byte window key and the per-slot
// decisions of one refinement round, shared by the kernels (gx_kernels.hip)
// and tools/strkey_check.cpp.
//
// Order (utf8mb4_bin PAD SPACE, the oracle's cmpRows): the effective string
// is the row's bytes with trailing 0x20 trimmed; unsigned bytes compare, and
// on a common prefix the shorter string sorts first. 0x00 is data:
// "ab" < "ab\0". A NULL row has effective length 0; its bytes are never read.
//
// Window key of round r, a u64:
//   bits 63..8  bytes 7r .. 7r+6 of the effective string, big-endian,
//               zero-padded
//   bits  7..0  c = clamp(elen - 7r, 0, 7), the number of bytes present
// Comparing W(.,0), W(.,1), ... lexicographically is the order above: two
// windows with the same c compare as their bytes; with different c the
// shorter one either differs in a present byte or is a zero-padded prefix of
// the longer, and then the count byte decides ("ab" vs "ab\0": equal byte
// fields, c = 2 < 3). A row with c < 7 has ended: whatever ties with it on
// every window so far is equal to it. A string that ends on a window edge
// has c == 7 and W == 0 in the next round, below every continuation.
//
// Bytes are reached through `byteAt(i)`, i an index into the column's data;
// strKeyWindow calls it only for s <= i < s + elen.
#ifndef GX_STRKEY_H
#define GX_STRKEY_H

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define GX_SK_HD __host__ __device__
#else
#define GX_SK_HD
#endif

namespace gxp {

constexpr int kStrKeyWin = 7;  // string bytes per window key

// effective length of the len bytes at s: trailing spaces trimmed
template <class ByteAt>
GX_SK_HD inline int64_t strKeyTrimLen(const ByteAt& byteAt, int64_t s,
                                      int64_t len) {
  while (len > 0 && byteAt(s + len - 1) == 0x20) len--;
  return len;
}

// rounds that can have active rows: a row is active in round r > 0 only if
// its window r-1 was full, elen >= 7r
GX_SK_HD inline uint32_t strKeyMaxRounds(uint32_t maxElen) {
  return maxElen / kStrKeyWin + 1;
}

template <class ByteAt>
GX_SK_HD inline uint64_t strKeyWindow(const ByteAt& byteAt, int64_t s,
                                      uint32_t elen, uint32_t round) {
  uint64_t first = (uint64_t)round * kStrKeyWin;
  if (first >= elen) return 0;
  uint64_t left = elen - first;
  int c = left < (uint64_t)kStrKeyWin ? (int)left : kStrKeyWin;
  uint64_t w = 0;
  for (int j = 0; j < c; j++)
    w |= (uint64_t)byteAt(s + (int64_t)first + j) << (56 - 8 * j);
  return w | (uint64_t)c;
}

GX_SK_HD inline int strKeyCount(uint64_t w) { return (int)(w & 0xFF); }

// ---- one refinement round, after the active rows of every tied segment
// stand in window order. Slot j of the active list has segment id seg[j]
// (non-decreasing along the list) and window key w[j]; m slots.

// slot j starts a run of equal keys inside its segment: a new segment head
template <class Seg, class Win>
GX_SK_HD inline bool strKeyIsHead(const Seg& seg, const Win& w, int64_t j) {
  return j == 0 || seg[j] != seg[j - 1] || w[j] != w[j - 1];
}

// slot j stays active: its run has more than one row and their windows were
// full. (Every row of a run shares w, so whole runs stay or leave.)
template <class Seg, class Win>
GX_SK_HD inline bool strKeyStaysActive(const Seg& seg, const Win& w, int64_t j,
                                       int64_t m) {
  if (strKeyCount(w[j]) < kStrKeyWin) return false;
  if (!strKeyIsHead(seg, w, j)) return true;
  return j + 1 < m && !strKeyIsHead(seg, w, j + 1);
}

// ---- f64 sort key: IEEE bits, -0.0 first mapped to +0.0 (they tie under
// `<`), complemented when negative, else the sign bit set. NaN order is
// unspecified (the oracle's `<` is no strict weak order there).
GX_SK_HD inline uint64_t f64OrderKey(uint64_t bits) {
  if (bits == 0x8000000000000000ULL) bits = 0;
  return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ULL);
}

}  // namespace gxp

#endif  // GX_STRKEY_H
