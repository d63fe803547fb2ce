// gx_units.h — width choice, pack and unpack of narrowed decimal units
// columns. A units column holds one two's-complement value
// per row at the narrowest of 1, 2, 4 or 8 bytes that holds the column's
// proven range (no bias; NULL rows hold 0). Included by the engine, by the
// device code (gx_device.h, the hipRTC-generated kernels) and by the
// stand-alone host check tools/units_narrow_check.cpp, so the check runs the
// functions that ship.
#ifndef GX_UNITS_H
#define GX_UNITS_H

#include <cstdint>

#if defined(__HIP__)
#define GX_HD __host__ __device__
#else
#define GX_HD
#endif

namespace gxp {

// narrowest signed width in {1, 2, 4, 8} bytes for values in [lo, hi]. The
// one-byte class is the symmetric [-127, 127]: a column whose minimum is
// exactly -128 takes two bytes (any width that holds the range is correct;
// this costs such a column one byte per row and nothing else). The 2 and
// 4 byte classes use their full two's-complement range.
GX_HD inline int unitsWidthFor(int64_t lo, int64_t hi) {
  if (lo >= -127 && hi <= 127) return 1;
  if (lo >= -32768 && hi <= 32767) return 2;
  if (lo >= -2147483648LL && hi <= 2147483647LL) return 4;
  return 8;
}

// width class of one value: the per-row form of unitsWidthFor. A column's
// width is the maximum class over its non-NULL rows.
GX_HD inline int unitsWidthOf(int64_t v) { return unitsWidthFor(v, v); }

// store v as element `row` of a column of `width` bytes (v must fit)
GX_HD inline void unitsStore(void* buf, int width, int64_t row, int64_t v) {
  switch (width) {
    case 1: ((int8_t*)buf)[row] = (int8_t)v; break;
    case 2: ((int16_t*)buf)[row] = (int16_t)v; break;
    case 4: ((int32_t*)buf)[row] = (int32_t)v; break;
    default: ((int64_t*)buf)[row] = v; break;
  }
}

// ---- unpack from the 32-bit words of a wide load (little endian) ----
// `k` is the element's index inside ITS word (1 B: 0..3, 2 B: 0..1)
GX_HD inline int64_t unitsUnpack1(uint32_t word, int k) {
  return (int64_t)(int8_t)(uint8_t)(word >> (8 * k));
}
GX_HD inline int64_t unitsUnpack2(uint32_t word, int k) {
  return (int64_t)(int16_t)(uint16_t)(word >> (16 * k));
}
GX_HD inline int64_t unitsUnpack4(uint32_t word) {
  return (int64_t)(int32_t)word;
}
GX_HD inline int64_t unitsUnpack8(uint32_t lo, uint32_t hi) {
  return (int64_t)((uint64_t)lo | ((uint64_t)hi << 32));
}

// bytes of a units buffer of n rows: rounded up to 16 B so a K-row vector
// load of the last full block never leaves the allocation's granule
GX_HD inline uint64_t unitsAllocBytes(int64_t nRows, int width) {
  return (((uint64_t)nRows * (uint64_t)width) + 15u) & ~(uint64_t)15u;
}

}  // namespace gxp

#endif  // GX_UNITS_H
