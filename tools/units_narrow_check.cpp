// Host-only check of gx_units.h, the functions behind the narrowed decimal
// units columns: the width choice from (min, max), the store
// and sign-extending unpack at every width, and the K-row unpack of each
// packed load word, against plain int64_t. Stand-alone: needs no GPU and no
// HIP; the device code and the generated kernels include the same header.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -I tidb_amd/csrc tools/units_narrow_check.cpp -o units_narrow_check
//   ./units_narrow_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gx_units.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      failures++;                                                 \
    }                                                             \
  } while (0)

static const int kWidths[] = {1, 2, 4, 8};

// element k of a run of `width`-byte values held as consecutive 32-bit words:
// the word and sub-word selection the generated blocked kernels spell out as
// literals (gx_jit.cpp, emitFetchBlk). This is a restatement: the program
// runs the shipped unitsUnpack1/2/4/8, NOT the generator's own
// indexing, which only the GPU tests cover.
static int64_t unitsUnpackAt(const uint32_t* words, int width, int k) {
  switch (width) {
    case 1: return gxp::unitsUnpack1(words[k >> 2], k & 3);
    case 2: return gxp::unitsUnpack2(words[k >> 1], k & 1);
    case 4: return gxp::unitsUnpack4(words[k]);
    default: return gxp::unitsUnpack8(words[2 * k], words[2 * k + 1]);
  }
}

// the boundary values of every width, each with its neighbours
static std::vector<int64_t> boundaries() {
  std::vector<int64_t> v = {0, 1, -1};
  for (int bits : {7, 8, 15, 16, 31, 32, 62}) {
    const int64_t p = (int64_t)1 << bits;
    for (int64_t d = -2; d <= 2; d++) {
      v.push_back(p + d);
      v.push_back(-p + d);
    }
  }
  v.push_back(INT64_MAX);
  v.push_back(INT64_MAX - 1);
  v.push_back(INT64_MIN);
  v.push_back(INT64_MIN + 1);
  return v;
}

// the one-byte class is [-127, 127] (see unitsWidthFor); 2 and 4 bytes take
// their full two's-complement range
static int refWidth(int64_t lo, int64_t hi) {
  for (int w : {1, 2, 4}) {
    const int64_t top = ((int64_t)1 << (8 * w - 1)) - 1;
    const int64_t bot = w == 1 ? -top : -top - 1;
    if (lo >= bot && hi <= top) return w;
  }
  return 8;
}

static void checkWidthChoice() {
  // the cases of the width-boundary test: extreme units -> width
  const struct { int64_t v; int w; } cases[] = {
      {127, 1}, {128, 2}, {-128, 2}, {-129, 2}, {32767, 2}, {32768, 4},
      {-32768, 2}, {-32769, 4}, {2147483647LL, 4}, {2147483648LL, 8},
      {-2147483648LL, 4}, {-2147483649LL, 8}};
  for (const auto& c : cases) {
    CHECK(gxp::unitsWidthOf(c.v) == c.w);
    CHECK(gxp::unitsWidthFor(c.v < 0 ? c.v : 0, c.v < 0 ? 0 : c.v) == c.w);
  }
  const std::vector<int64_t> b = boundaries();
  for (int64_t lo : b)
    for (int64_t hi : b) {
      if (lo > hi) continue;
      const int w = gxp::unitsWidthFor(lo, hi);
      CHECK(w == refWidth(lo, hi));
      // the range's width is the larger of its ends' classes
      const int wl = gxp::unitsWidthOf(lo), wh = gxp::unitsWidthOf(hi);
      CHECK(w == (wl > wh ? wl : wh));
    }
  // synthetic lineitem ranges at frac 2
  CHECK(gxp::unitsWidthFor(100, 5000) == 2);
  CHECK(gxp::unitsWidthFor(90100, 10495000) == 4);
  CHECK(gxp::unitsWidthFor(0, 10) == 1);
  CHECK(gxp::unitsWidthFor(0, 8) == 1);
}

// store `vals` at `width`, then read every element back through the K-row
// word unpack for each K (the buffer is exactly the bytes the values take,
// on the heap, so a sanitizer sees any access outside it)
static void roundTrip(const std::vector<int64_t>& vals, int width) {
  const size_t n = vals.size();
  std::vector<uint8_t> heap(n * width);
  for (size_t i = 0; i < n; i++)
    gxp::unitsStore(heap.data(), width, (int64_t)i, vals[i]);
  for (int K : {1, 2, 4}) {
    const size_t blkBytes = (size_t)K * width;
    for (size_t base = 0; base + K <= n; base += K) {
      // a lane's load: K * width bytes, held as 32-bit words (a load shorter
      // than a word is zero-extended into one, as a sub-dword load is)
      uint32_t words[8] = {0};
      std::memcpy(words, heap.data() + base * width, blkBytes);
      for (int k = 0; k < K; k++)
        CHECK(unitsUnpackAt(words, width, k) == vals[base + k]);
    }
  }
}

static void checkPackUnpack() {
  std::mt19937_64 rng(20260105);
  for (int width : kWidths) {
    const int64_t top =
        width == 8 ? INT64_MAX : ((int64_t)1 << (8 * width - 1)) - 1;
    const int64_t bot = -top - 1;
    std::vector<int64_t> vals;
    for (int64_t v : boundaries())
      if (v >= bot && v <= top) vals.push_back(v);
    if (width == 1)  // exhaustive
      for (int64_t v = bot; v <= top; v++) vals.push_back(v);
    if (width == 2)
      for (int64_t v = bot; v <= top; v += 1) vals.push_back(v);
    std::uniform_int_distribution<int64_t> dist(bot, top);
    for (int i = 0; i < 4096; i++) vals.push_back(dist(rng));
    while (vals.size() % 4) vals.push_back(0);
    roundTrip(vals, width);
    // every value of the width's range chooses a width no larger (-128 is
    // stored and read back at one byte above, but never chosen into it)
    for (int64_t v : vals)
      if (v != -128) CHECK(gxp::unitsWidthOf(v) <= width);
  }
  // single-word forms
  CHECK(gxp::unitsUnpack1(0x80FF7F01u, 0) == 1);
  CHECK(gxp::unitsUnpack1(0x80FF7F01u, 1) == 127);
  CHECK(gxp::unitsUnpack1(0x80FF7F01u, 2) == -1);
  CHECK(gxp::unitsUnpack1(0x80FF7F01u, 3) == -128);
  CHECK(gxp::unitsUnpack2(0x80007FFFu, 0) == 32767);
  CHECK(gxp::unitsUnpack2(0x80007FFFu, 1) == -32768);
  CHECK(gxp::unitsUnpack4(0x80000000u) == -2147483648LL);
  CHECK(gxp::unitsUnpack8(0u, 0x80000000u) == INT64_MIN);
  CHECK(gxp::unitsUnpack8(0xFFFFFFFFu, 0x7FFFFFFFu) == INT64_MAX);
}

static void checkAllocBytes() {
  for (int width : kWidths)
    for (int64_t n : {1, 3, 4, 5, 15, 16, 17, 5000, 599860520}) {
      const uint64_t b = gxp::unitsAllocBytes(n, width);
      CHECK(b % 16 == 0);
      CHECK(b >= (uint64_t)n * width && b < (uint64_t)n * width + 16);
    }
}

int main() {
  checkWidthChoice();
  checkPackUnpack();
  checkAllocBytes();
  if (failures) {
    fprintf(stderr, "units_narrow_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("units_narrow_check OK\n");
  return 0;
}
