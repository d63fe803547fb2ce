// Host-only check of the two functions between the compact result block and
// the row decode: gxp::collectCompactGroups (header -> occupied records, the
// kResultCap edge) and gxp::foldGroupSlot (accumulator-bank fold; the same
// function compactGroupsKernel runs on device), against an __int128
// reference. Stand-alone: needs no GPU and no HIP.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -I tidb_amd/csrc tools/result_fold_check.cpp -o result_fold_check
//   ./result_fold_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gx_common.h"

using gxp::FusedResultBlock;
using gxp::GroupSlot;
using gxp::kMaxAggs;
using gxp::kResultCap;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      failures++;                                                 \
    }                                                             \
  } while (0)

static void checkCollect() {
  auto blk = std::make_unique<FusedResultBlock>();
  std::memset(blk.get(), 0, sizeof(*blk));
  for (int i = 0; i < kResultCap; i++) blk->slots[i].key = 1000 + i;
  for (uint32_t n : {0u, 1u, (uint32_t)kResultCap - 1, (uint32_t)kResultCap}) {
    blk->hdr.nOccupied = n;
    std::vector<const GroupSlot*> occ;
    CHECK(gxp::collectCompactGroups(*blk, &occ));
    CHECK(occ.size() == n);
    for (uint32_t i = 0; i < n; i++) CHECK(occ[i]->key == 1000 + i);
  }
  // the cursor counts every occupied slot, also those that found no room
  for (uint32_t n : {(uint32_t)kResultCap + 1, 8192u, 0xFFFFFFFFu}) {
    blk->hdr.nOccupied = n;
    std::vector<const GroupSlot*> occ;
    CHECK(!gxp::collectCompactGroups(*blk, &occ));
    CHECK(occ.empty());
  }
}

static void checkFold() {
  std::mt19937_64 rng(7);
  const int32_t kinds[kMaxAggs] = {0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 0, 0};
  // words that force carries out of accLo and both signs of accHi
  const uint64_t edge[] = {0, 1, ~0ULL, ~0ULL - 1, 1ULL << 63,
                           (1ULL << 63) - 1, 0x7CE66C50E2840000ULL};
  for (int iter = 0; iter < 2000; iter++) {
    const int nAcc = 1 + (int)(rng() % kMaxAggs);
    const int nCnt = 1 + (int)(rng() % kMaxAggs);
    GroupSlot banks[16];
    auto word = [&]() {
      return rng() % 3 ? edge[rng() % (sizeof(edge) / sizeof(edge[0]))] : rng();
    };
    for (auto& b : banks) {
      b.key = 5;
      for (int s = 0; s < kMaxAggs; s++) {
        b.accLo[s] = word();
        b.accHi[s] = rng() % 2 ? (int64_t)word() : (int64_t)(rng() % 3) - 1;
        b.cnt[s] = (int64_t)(rng() % 100000);
        if (kinds[s] == 3) {
          double x = (double)(int64_t)(rng() % 2000001) - 1e6;
          std::memcpy(&b.accLo[s], &x, 8);
        }
      }
    }
    GroupSlot got = banks[0], want = banks[0];
    for (int k = 1; k < 16; k++)
      gxp::foldGroupSlot(got, banks[k], nAcc, kinds, nCnt);
    for (int s = 0; s < kMaxAggs; s++) {
      if (s < nAcc) {
        if (kinds[s] == 0) {
          unsigned __int128 v = 0;
          for (auto& b : banks)
            v += ((unsigned __int128)(uint64_t)b.accHi[s] << 64) | b.accLo[s];
          want.accLo[s] = (uint64_t)v;
          want.accHi[s] = (int64_t)(uint64_t)(v >> 64);
        } else if (kinds[s] == 3) {
          double x;
          std::memcpy(&x, &banks[0].accLo[s], 8);
          for (int k = 1; k < 16; k++) {
            double y;
            std::memcpy(&y, &banks[k].accLo[s], 8);
            x += y;
          }
          std::memcpy(&want.accLo[s], &x, 8);
        } else {
          for (auto& b : banks)
            if (b.accLo[s] > want.accLo[s]) want.accLo[s] = b.accLo[s];
        }
      }
      if (s < nCnt) {
        want.cnt[s] = 0;
        for (auto& b : banks) want.cnt[s] += b.cnt[s];
      }
    }
    // words beyond nAcc / nCnt are not the plan's: left alone
    CHECK(std::memcmp(&got, &want, sizeof(got)) == 0);
  }
}

int main() {
  checkCollect();
  checkFold();
  if (failures) {
    fprintf(stderr, "result_fold_check: %d failure(s)\n", failures);
    return 1;
  }
  printf("result_fold_check OK (cap %d)\n", kResultCap);
  return 0;
}
