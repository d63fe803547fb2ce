// tidb_amd/csrc/gx_kernels.hip — MI355X (gfx950/CDNA4) kernels for the
// TiDB analytical hot path.
//
// Fused scan -> filter -> project -> hash-aggregate in ONE pass over the
// columns (the MI355X-native form of SelectionExec -> ProjectionExec ->
// HashAggExec, pkg/executor/select.go:750 / projection.go:77 /
// aggregate/agg_hash_*.go): every consumed input column is read once from
// HBM — the path is HBM-bandwidth-bound (no MFMA shape here).
//
// Grouping: per-workgroup LDS hash table (LDS-staged accumulator state,
// atomically updated), flushed once per workgroup into a global table with
// device-scope atomics — the device analog of the reference's partial/final
// worker split (agg_hash_executor.go:54-92).
//
// Decimal arithmetic: fixed-point int64/int128 units at static scales; exact,
// with overflow detection -> error flag (never silent). Equivalence to the
// word-based MyDecimal arithmetic is covered by tests/golden + parity suites.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <hipcub/hipcub.hpp>
#include "gx_device.h"

#include "gx_common.h"

namespace gxp {

// ------------------------------------------------------------------
// shared PRNG/date spec — MUST generate bit-identical data to the CPU
// restatement in oracle/tpch.cpp (parity-tested).
// ------------------------------------------------------------------
__host__ __device__ inline uint64_t fieldRand(uint64_t seed, int64_t row, int field) {
  uint64_t h = splitmix64(seed ^ (0x9E3779B97F4A7C15ULL * (uint64_t)(row + 1)));
  return splitmix64(h ^ (0xBF58476D1CE4E5B9ULL * (uint64_t)(field + 1)));
}
__host__ __device__ inline int64_t daysFromCivil(int y, int m, int d) {
  y -= m <= 2;
  int64_t era = (y >= 0 ? y : y - 399) / 400;
  unsigned yoe = (unsigned)(y - era * 400);
  unsigned doy = (unsigned)((153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1);
  unsigned doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (int64_t)doe - 719468;
}
__host__ __device__ inline void civilFromDays(int64_t z, int* yy, int* mm, int* dd) {
  z += 719468;
  int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  unsigned doe = (unsigned)(z - era * 146097);
  unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  int64_t y = (int64_t)yoe + era * 400;
  unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  unsigned mp = (5 * doy + 2) / 153;
  unsigned d = doy - (153 * mp + 2) / 5 + 1;
  unsigned m = mp < 10 ? mp + 3 : mp - 9;
  *yy = (int)(y + (m <= 2));
  *mm = (int)m;
  *dd = (int)d;
}

// packed CoreTime DATE (time.go:235-251,266: fspTt 0b1110 marks TypeDate)
__host__ __device__ inline uint64_t timeFromDate(int y, int m, int d) {
  return ((uint64_t)y << 50) | ((uint64_t)m << 46) | ((uint64_t)d << 41) | 0xEULL;
}

// date-range constants are computed (constant-folded), never hand-written
#define GX_EPOCH_1992 daysFromCivil(1992, 1, 1)
#define GX_SHIPDATE_DAYS (daysFromCivil(1998, 12, 1) - daysFromCivil(1992, 1, 1) + 1)
#define GX_ORDERDATE_DAYS (daysFromCivil(1998, 8, 2) - daysFromCivil(1992, 1, 1) + 1)

// canonical cents -> 40-byte MyDecimal (scale 2), matches oracle/tpch.cpp
__device__ inline void storeDecCents(uint8_t* p, int64_t cents) {
  int64_t ip = cents / 100;
  uint32_t f = (uint32_t)(cents % 100);
  int digits = 1;
  for (int64_t t = ip; t >= 10; t /= 10) digits++;
  uint32_t hdr = (uint32_t)(uint8_t)digits | (2u << 8) | (2u << 16);
  uint32_t* w = (uint32_t*)p;
  w[0] = hdr;
  w[1] = (uint32_t)ip;
  w[2] = f * 10000000u;
  w[3] = 0; w[4] = 0; w[5] = 0; w[6] = 0; w[7] = 0; w[8] = 0; w[9] = 0;
}

// ------------------------------------------------------------------
// lineitem generator: cols 0..7 =
//   orderkey i64, quantity dec, extendedprice dec, discount dec, tax dec,
//   returnflag char(1), linestatus char(1), shipdate date
// ------------------------------------------------------------------
__global__ void genLineitemKernel(DevTable tab, int64_t rowBegin, int64_t nRows,
                                  uint64_t seed, int64_t totalRows) {
  int64_t nOrders = totalRows / 4;
  if (nOrders < 1) nOrders = 1;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nRows;
       i += stride) {
    int64_t row = rowBegin + i;
    ((int64_t*)tab.cols[0].data)[i] =
        1 + (int64_t)(fieldRand(seed, row, 0) % (uint64_t)nOrders);
    storeDecCents((uint8_t*)tab.cols[1].data + i * 40,
                  (1 + (int64_t)(fieldRand(seed, row, 1) % 50)) * 100);
    storeDecCents((uint8_t*)tab.cols[2].data + i * 40,
                  90100 + (int64_t)(fieldRand(seed, row, 2) % (10495000 - 90100 + 1)));
    storeDecCents((uint8_t*)tab.cols[3].data + i * 40,
                  (int64_t)(fieldRand(seed, row, 3) % 11));
    storeDecCents((uint8_t*)tab.cols[4].data + i * 40,
                  (int64_t)(fieldRand(seed, row, 4) % 9));
    const char rf[3] = {'A', 'N', 'R'};
    ((uint8_t*)tab.cols[5].data)[i] = rf[fieldRand(seed, row, 5) % 3];
    tab.cols[5].offsets[i + 1] = i + 1;
    const char ls[2] = {'O', 'F'};
    ((uint8_t*)tab.cols[6].data)[i] = ls[fieldRand(seed, row, 6) % 2];
    tab.cols[6].offsets[i + 1] = i + 1;
    int y, m, d;
    civilFromDays(GX_EPOCH_1992 +
                      (int64_t)(fieldRand(seed, row, 7) % (uint64_t)GX_SHIPDATE_DAYS),
                  &y, &m, &d);
    ((uint64_t*)tab.cols[7].data)[i] = timeFromDate(y, m, d);
    if (i == 0) {
      tab.cols[5].offsets[0] = 0;
      tab.cols[6].offsets[0] = 0;
    }
  }
}

// ------------------------------------------------------------------
// fused filter+project+aggregate
// ------------------------------------------------------------------
//
// Two instantiations: NARROW (int64 VM registers — covers every value with
// <= 18 significant digits, i.e. all real decimal(15,2)-class workloads) and
// WIDE (int128). NARROW detects overflow per operation and sets the
// RETRY_WIDE flag; the engine then relaunches the WIDE variant — exactness
// is never traded away.



// per-row pipeline after the raw fetch: filter -> VM -> LDS aggregate.
// Returns false on a hard failure (error flag already set). OPS is the VM
// opcode set compiled into this variant (gx_vm.h vmStep).
template <bool WIDE, uint32_t OPS, typename VMT, bool WK = false, typename RAWT>
__device__ __attribute__((always_inline)) inline bool processRow(const FusedQueryDesc& d, int64_t row,
                                  const RAWT& raw, Lds3GroupSlot* lds,
                                  uint64_t* mySel,
                                  WkLds64* wkCacheH = nullptr,
                                  WkLds32* wkCacheS = nullptr) {
  // ---- filter (CNF of OR groups; NULL rejects — expression.go:507
  // toBool; a disjunctive conjunct passes when ANY member does) ----
  bool hardFail = false;
  auto evalOne = [&](const PredDesc& pd) -> bool {
    const DevCol& c = d.table.cols[pd.col];
    if (pd.kind == PRED_IS_NULL)  // null bit is the result; no null-reject
      return colIsNull(c, row) == (pd.cmp == 4 /*GX_F_EQ*/);
    if (colIsNull(c, row)) return false;
    if (pd.kind == PRED_TIME_CMP_CONST) {
      uint64_t v = raw.get(pd.slot).x & ~0xFULL;
      uint64_t k = pd.constU64 & ~0xFULL;
      return cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
    }
    if (pd.kind == PRED_I64_CMP_CONST) {
      int64_t v = (int64_t)raw.get(pd.slot).x;
      int64_t k = (int64_t)pd.constU64;
      return cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
    }
    if (pd.kind == PRED_DEC_CMP_CONST) {
      typename VT<WIDE>::T u;
      int sc;
      if (pd.slot >= 0 && d.fetch[pd.slot].kind == FETCH_UNITS8) {
        // proven column: the slot already holds the units at the column frac
        u = VT<WIDE>::fromI64((int64_t)raw.get(pd.slot).x, nullptr);
      } else if (!loadDecimalUnits<WIDE>((const uint8_t*)c.data + row * 40, &u,
                                         &sc, d.errorFlag)) {
        hardFail = true;
        return false;
      }
      int cmp = VT<WIDE>::cmp(u, VT<WIDE>::fromI64((int64_t)pd.constU64, nullptr));
      return cmpResult(cmp, pd.cmp);
    }
    // string EQ/NE const + LIKE-'prefix%' (per-pred inline const)
    return evalSimplePred(d.table, pd, pd.strC, pd.strCLen, row);
  };
  bool pass = true;
  for (int p = 0; p < d.nPreds && pass;) {
    int ng = d.preds[p].orWith + 1;
    bool ok = false;
    for (int j = 0; j < ng && !ok; j++) ok = evalOne(d.preds[p + j]);
    if (hardFail) return false;
    pass = ok;
    p += ng;
  }
  if (!pass) return true;
  (*mySel)++;
  if (d.ablate == 2) return true;  // timing ablation: filter only

  // ---- projection / agg-arg VM ----
  VMT vm;
  vm.nullBits = 0;
  bool bad = false;
  bool ovf = false;
  for (int i = 0; i < d.nIns && !bad; i++) {
    const VmIns& ins = d.ins[i];
    switch (ins.op) {
      case VM_LOAD_DEC: {
        const DevCol& c = d.table.cols[ins.a];
        bool nul = colIsNull(c, row);
        typename VT<WIDE>::T v = VT<WIDE>::zero();
        if (!nul && d.fetch[ins.c].kind == FETCH_UNITS8) {
          // proven column: units at scale ins.b, sign-extended when WIDE
          v = VT<WIDE>::fromI64((int64_t)raw.get(ins.c).x, nullptr);
        } else if (!nul) {
          int sc;
          if (!parseDecimalRaw<WIDE>(raw.get(ins.c), &v, &sc, d.errorFlag,
                                     ins.b, d.insP10[i], d.insMagic[i])) {
            bad = true;
            break;
          }
          if (sc != ins.b) {  // engine encoded expected scale in b
            if (sc < ins.b) v = VT<WIDE>::scale10(v, ins.b - sc, &ovf);
            else { atomicOr(d.errorFlag, kErrScale); bad = true; break; }
          }
        }
        vm.set(ins.dst, v);
        vm.setNull(ins.dst, nul);
        break;
      }
      case VM_LOAD_I64: {
        const DevCol& c = d.table.cols[ins.a];
        bool nul = colIsNull(c, row);
        vm.set(ins.dst, nul ? VT<WIDE>::zero()
                            : VT<WIDE>::fromI64((int64_t)raw.get(ins.c).x, &ovf));
        vm.setNull(ins.dst, nul);
        break;
      }
      case VM_STRLEN: {
        // LENGTH (builtinLengthSig): byte length from the offsets pair
        const DevCol& c = d.table.cols[ins.a];
        bool nul = colIsNull(c, row);
        ulonglong2 off = raw.get(ins.c);
        int64_t len = c.denseOffsets ? 1 : (int64_t)(off.y - off.x);
        vm.set(ins.dst, nul ? VT<WIDE>::zero() : VT<WIDE>::fromI64(len, &ovf));
        vm.setNull(ins.dst, nul);
        break;
      }
      case VM_LIKE: {
        // LIKE / NOT LIKE in value context: i64 0/1, NULL string -> NULL
        // (offsets and bytes load at use, not through the fetch pipeline)
        const DevCol& c = d.table.cols[ins.a];
        bool nul = colIsNull(c, row);
        int64_t r = 0;
        if (!nul)
          r = likeColMatch(c, d.likePats[ins.b], row) != (ins.c != 0) ? 1 : 0;
        vm.set(ins.dst, VT<WIDE>::fromI64(r, &ovf));
        vm.setNull(ins.dst, nul);
        break;
      }
      default:
        if (!vmStep<WIDE, OPS>(vm, ins, d.insP10[i], d.constLo, d.constHi,
                               d.errorFlag, &ovf))
          bad = true;
        break;
    }
  }
  if (ovf) {
    atomicOr(d.errorFlag, WIDE ? kErrOverflow : kErrRetryWide);
    return false;
  }
  if (bad) return false;

  if (d.ablate == 1) {  // timing ablation: keep VM results live, skip agg
    uint64_t sink = 0;
    for (int a = 0; a < d.nAggs; a++)
      if (d.aggs[a].srcReg >= 0)
        sink ^= (uint64_t)VT<WIDE>::toAcc(vm.get(d.aggs[a].srcReg)).lo;
    asm volatile("" ::"v"(sink));
    return true;
  }

  // ---- group lookup / insert (LDS table, or global when NDV > kLdsGroups) ----
  // Wide serialized keys resolve the GLOBAL slot first (hash probe + record
  // verify); the LDS stage then keys on that slot index — exact, and the
  // flush adds straight into globalTable[slot].
  uint64_t key;
  uint32_t gslot = 0;
  if constexpr (WK) {
    if (d.ablate == 4) {  // timing ablation: fake slots, skip resolution
      gslot = (uint32_t)(splitmix64((uint64_t)row) & 255u);
    } else if (!makeWideGroupKey<WIDE>(d, row, raw, vm, wkCacheH, wkCacheS,
                                       &gslot)) {
      return false;
    }
    if (d.ablate == 3) {  // timing ablation: resolve keys, skip accumulate
      asm volatile("" ::"v"(gslot));
      return true;
    }
    key = gslot;
  } else {
    if (!makeGroupKey(d, row, raw, &key, d.errorFlag)) return false;
  }
  if (!d.noLds) {
    uint32_t slot = (uint32_t)(splitmix64(key) & (kLdsGroups - 1));
    for (int probe = 0;; probe++) {
      if (probe >= kLdsGroups) {
        atomicOr(d.errorFlag, kErrLdsFull);
        return false;
      }
      uint64_t cur = lds[slot].key;
      if (cur == key) break;
      if (cur == kEmptyKey) {
        uint64_t prev = lds3CasKey(&lds[slot], kEmptyKey, key);
        if (prev == kEmptyKey || prev == key) break;
      }
      slot = (slot + 1) & (kLdsGroups - 1);
    }
    Lds3GroupSlot* target = &lds[slot];
    // ---- update states: one atomic per unique acc, one or per-agg counts ----
    if (d.sharedCnt) lds3AccumCnt(target, 0, 1);
    for (int s = 0; s < d.nAccSlots; s++) {
      int reg = d.accReg[s];
      if (d.accKind[s] == 3) {  // f64 sum: raw column bits, f64 LDS atomic
        const DevCol& fc = d.table.cols[d.accFcol[s]];
        if (colIsNull(fc, row)) continue;
        lds3AccumF64(target, s, __builtin_bit_cast(double, raw.get(reg).x));
        continue;
      }
      if (vm.isNull(reg)) continue;
      if (d.accKind[s] == 0) {
        lds3AccumAcc(target, s, VT<WIDE>::toAcc(vm.get(reg)));
      } else {
        Int128 v = VT<WIDE>::toAcc(vm.get(reg));
        bool fits = (v.hi == 0 && (int64_t)v.lo >= 0) ||
                    (v.hi == -1 && (int64_t)v.lo < 0);
        if (WIDE && !fits) {
          atomicOr(d.errorFlag, kErrOverflow);  // >64-bit min/max value
          return false;
        }
        uint64_t enc = biasI64((int64_t)v.lo);
        lds3AccumMax(target, s, d.accKind[s] == 2 ? ~enc : enc);
      }
    }
    if (!d.sharedCnt) {
      for (int a = 0; a < d.nAggs; a++) {
        const AggDesc& ad = d.aggs[a];
        if (ad.fr >= 0) continue;  // firstrow(group col): no per-row state
        bool isNull = ad.fcol >= 0
                          ? colIsNull(d.table.cols[ad.fcol], row)
                          : (ad.srcReg >= 0 && vm.isNull(ad.srcReg));
        if (!isNull) lds3AccumCnt(target, a, 1);
      }
    }
    return true;
  }
  // global-direct path (mid/high NDV; table grows on kErrGlobalFull retry)
  uint32_t slot;
  if constexpr (WK) {
    slot = gslot;  // makeWideGroupKey already resolved (and claimed) the slot
  } else {
    uint32_t gmask = (1u << d.globalGroupsLog2) - 1;
    slot = (uint32_t)(splitmix64(key) & gmask);
    for (uint32_t probe = 0;; probe++) {
      if (probe > gmask) {
        atomicOr(d.errorFlag, kErrGlobalFull);
        return false;
      }
      uint64_t cur = d.globalTable[slot].key;
      if (cur == key) break;
      if (cur == kEmptyKey) {
        uint64_t prev = atomicCAS((unsigned long long*)&d.globalTable[slot].key,
                                  (unsigned long long)kEmptyKey,
                                  (unsigned long long)key);
        if (prev == kEmptyKey || prev == key) break;
      }
      slot = (slot + 1) & gmask;
    }
  }
  GroupSlot* target =
      &d.globalTable[slot + ((uint32_t)blockIdx.x & (d.accBanks - 1)) *
                                (int64_t)(1u << d.globalGroupsLog2)];
  if (d.sharedCnt) accumInto(target, 0, Int128{0, 0}, 1);  // bumps cnt[0] only
  for (int s = 0; s < d.nAccSlots; s++) {
    int reg = d.accReg[s];
    if (d.accKind[s] == 3) {  // f64 sum
      const DevCol& fc = d.table.cols[d.accFcol[s]];
      if (colIsNull(fc, row)) continue;
      atomicAdd((double*)&target->accLo[s],
                __builtin_bit_cast(double, raw.get(reg).x));
      continue;
    }
    if (vm.isNull(reg)) continue;
    if (d.accKind[s] == 0) {
      accumInto(target, s, VT<WIDE>::toAcc(vm.get(reg)), 0);
    } else {
      Int128 v = VT<WIDE>::toAcc(vm.get(reg));
      bool fits = (v.hi == 0 && (int64_t)v.lo >= 0) ||
                  (v.hi == -1 && (int64_t)v.lo < 0);
      if (WIDE && !fits) {
        atomicOr(d.errorFlag, kErrOverflow);
        return false;
      }
      uint64_t enc = biasI64((int64_t)v.lo);
      accumMax(target, s, d.accKind[s] == 2 ? ~enc : enc);
    }
  }
  if (!d.sharedCnt) {
    for (int a = 0; a < d.nAggs; a++) {
      const AggDesc& ad = d.aggs[a];
      if (ad.fr >= 0) continue;  // firstrow(group col): no per-row state
      bool isNull = ad.fcol >= 0
                        ? colIsNull(d.table.cols[ad.fcol], row)
                        : (ad.srcReg >= 0 && vm.isNull(ad.srcReg));
      if (!isNull) accumInto(target, a, Int128{0, 0}, 1);
    }
  }
  return true;
}

template <bool WIDE, int R, bool DIVOK = false, int NVM = 12, bool WK = false>
__launch_bounds__(256)
__global__ void fusedAggKernel(const FusedQueryDesc* __restrict__ dp) {
  const FusedQueryDesc& d = *dp;
  // any error flag dooms the whole pass (the engine discards it and either
  // retries or fails), so late blocks bail before fetching anything: a
  // doomed attempt (LdsFull probe, GlobalFull grow, packed->wide) costs
  // flag-propagation time instead of a full 60M-row pass
  if (__hip_atomic_load(d.errorFlag, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT))
    return;
  bool failed = false;
  __shared__ GroupSlot lds[kLdsGroups];
  Lds3GroupSlot* lds3 = (Lds3GroupSlot*)lds;
  // wide keys: the hash->slot resolution cache (exact; gx_device.h)
  __shared__ uint64_t wkH[WK ? kWkCache : 1];
  __shared__ uint32_t wkS[WK ? kWkCache : 1];
  WkLds64* wkCacheH = (WkLds64*)wkH;
  WkLds32* wkCacheS = (WkLds32*)wkS;
  if (WK)
    for (int i = threadIdx.x; i < kWkCache; i += blockDim.x) wkH[i] = ~0ULL;
  for (int i = threadIdx.x; i < kLdsGroups; i += blockDim.x) {
    lds[i].key = kEmptyKey;
    for (int a = 0; a < kMaxAggs; a++) {
      lds[i].accLo[a] = 0;
      lds[i].accHi[a] = 0;
      lds[i].cnt[a] = 0;
    }
  }
  __syncthreads();

  int64_t n = d.table.nRows;
  int64_t per = (n + gridDim.x - 1) / gridDim.x;
  int64_t begin = (int64_t)blockIdx.x * per;
  int64_t end = begin + per;
  if (end > n) end = n;
  uint64_t mySel = 0;

  // 2-deep software-pipelined grouped-fetch loop: row k+1's loads issue
  // before row k's pipeline runs, so every wave keeps ~2 rows of bytes in
  // flight (the kernel is HBM-latency bound: VALU util ~7%, concurrency =
  // waves x rows-in-flight). Two NAMED RawState structs, never indexed or
  // swapped through a pointer -- indexed access re-rolls to scratch spills
  // (measured 6.1 ms), this form stays in registers.
  {
    // R is the compile-time fetch-slot bound: 5 covers Q1-shaped queries at
    // one extra wave/SIMD of occupancy; 8 is the general variant.
    using RAWT = typename std::conditional<R <= 5, RawState5, RawState>::type;
    const int64_t stride = blockDim.x;
    int64_t row = begin + threadIdx.x;
    RAWT rawA, rawB;
    if (row < end) fetchRow(d.table, d.fetch, d.nFetch, row, rawA);
    for (; row < end && !failed; row += 2 * stride) {
      const int64_t rB = row + stride;
      if (rB < end) fetchRow(d.table, d.fetch, d.nFetch, rB, rawB);
      using VMT = typename std::conditional<NVM <= 12, VmState<WIDE>,
                                            VmState14<WIDE>>::type;
      // engine launches the DIVOK variant for plans containing DIV; in the
      // others a DIV is a dispatch bug and fails loudly
      constexpr uint32_t OPS = DIVOK ? kVmOpsFull : kVmOpsFull & ~(1u << VM_DIV);
      if (!processRow<WIDE, OPS, VMT, WK>(d, row, rawA, lds3, &mySel,
                                            wkCacheH, wkCacheS)) { failed = true; break; }
      const int64_t rA2 = row + 2 * stride;
      if (rA2 < end) fetchRow(d.table, d.fetch, d.nFetch, rA2, rawA);
      if (rB < end && !processRow<WIDE, OPS, VMT, WK>(d, rB, rawB, lds3, &mySel,
                                                        wkCacheH, wkCacheS)) failed = true;
    }
  }

  if (d.selCount) {
    // wave-level reduce then one atomic per wave (G12)
    uint64_t total = mySel;
    for (int off = 32; off > 0; off >>= 1)
      total += __shfl_down(total, off, 64);
    if ((threadIdx.x & 63) == 0 && total)
      atomicAdd((unsigned long long*)d.selCount, (unsigned long long)total);
  }
  __syncthreads();

  // ---- flush LDS table into the global table ----
  for (int i = threadIdx.x; i < kLdsGroups; i += blockDim.x) {
    if (lds[i].key == kEmptyKey) continue;
    uint64_t key = lds[i].key;
    uint32_t slot;
    bool ok = true;
    if constexpr (WK) {
      slot = (uint32_t)key;  // wide keys: the LDS key IS the global slot
    } else {
      uint32_t gmask = (1u << d.globalGroupsLog2) - 1;
      slot = (uint32_t)(splitmix64(key) & gmask);
      for (uint32_t probe = 0;; probe++) {
        if (probe > gmask) { atomicOr(d.errorFlag, kErrGlobalFull); ok = false; break; }
        uint64_t cur = d.globalTable[slot].key;
        if (cur == key) break;
        if (cur == kEmptyKey) {
          uint64_t prev = atomicCAS((unsigned long long*)&d.globalTable[slot].key,
                                    (unsigned long long)kEmptyKey,
                                    (unsigned long long)key);
          if (prev == kEmptyKey || prev == key) break;
        }
        slot = (slot + 1) & gmask;
      }
    }
    if (!ok) continue;
    for (int s = 0; s < d.nAccSlots; s++) {
      if (d.accKind[s] == 3) {  // f64 sum: add the LDS partial
        atomicAdd((double*)&d.globalTable[slot].accLo[s],
                  __builtin_bit_cast(double, lds[i].accLo[s]));
        continue;
      }
      if (d.accKind[s] != 0) {
        accumMax(&d.globalTable[slot], s, lds[i].accLo[s]);
        continue;
      }
      Int128 v = {lds[i].accLo[s], lds[i].accHi[s]};
      accumInto(&d.globalTable[slot], s, v, 0);
    }
    int nCnt = d.sharedCnt ? 1 : d.nAggs;
    for (int a = 0; a < nCnt; a++)
      accumInto(&d.globalTable[slot], a, Int128{0, 0}, lds[i].cnt[a]);
  }
}

__global__ void initGlobalTableKernel(GroupSlot* table, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  table[i].key = kEmptyKey;
  for (int a = 0; a < kMaxAggs; a++) {
    table[i].accLo[a] = 0;
    table[i].accHi[a] = 0;
    table[i].cnt[a] = 0;
  }
}

// One thread per bank-0 slot: an occupied slot (folded with banks 1+ when
// the noLds pass wrote them) is appended to out->slots through the header's
// cursor. A flagged pass is retried or fails on the host: nothing to append.
__launch_bounds__(256)
__global__ void compactGroupsKernel(const FusedQueryDesc* __restrict__ dp,
                                    int usedBanks, FusedResultBlock* out) {
  const FusedQueryDesc& d = *dp;
  if (out->hdr.errorFlag != 0) return;
  const int64_t nSlots1 = (int64_t)1 << d.globalGroupsLog2;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nSlots1) return;
  const GroupSlot* src = &d.globalTable[i];
  if (src->key == kEmptyKey) return;
  uint32_t at = atomicAdd(&out->hdr.nOccupied, 1u);
  if (at >= (uint32_t)kResultCap) return;
  GroupSlot rec = *src;
  const int nCnt = d.sharedCnt ? 1 : d.nAggs;
  for (int bank = 1; bank < usedBanks; bank++)
    foldGroupSlot(rec, d.globalTable[bank * nSlots1 + i], d.nAccSlots,
                  d.accKind, nCnt);
  out->slots[at] = rec;
}


// ==================================================================
// join-aggregate pipeline (Q3 class) — see gx_common.h JoinAggDesc
// ==================================================================

__device__ inline uint64_t hashKey(uint64_t k) { return splitmix64(k); }

__device__ inline void bloomSet(const JoinAggDesc& d, uint64_t key) {
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloomLog2) - 1;
  uint32_t b1 = (uint32_t)h & mask;
  uint32_t b2 = (uint32_t)(h >> 32) & mask;
  atomicOr(&d.bloom[b1 >> 5], 1u << (b1 & 31));
  atomicOr(&d.bloom[b2 >> 5], 1u << (b2 & 31));
}

__device__ inline void bloom0Set(const JoinAggDesc& d, uint64_t key) {
  if (d.bloom0Log2 == 0) return;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloom0Log2) - 1;
  atomicOr(&d.bloom0[((uint32_t)h & mask) >> 5], 1u << ((uint32_t)h & 31));
  atomicOr(&d.bloom0[((uint32_t)(h >> 32) & mask) >> 5],
           1u << ((uint32_t)(h >> 32) & 31));
}

__device__ inline bool bloom0MayHave(const JoinAggDesc& d, uint64_t key) {
  if (d.bloom0Log2 == 0) return true;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloom0Log2) - 1;
  uint32_t b1 = (uint32_t)h & mask;
  uint32_t b2 = (uint32_t)(h >> 32) & mask;
  auto bm = gptr<uint32_t>(d.bloom0);
  if (!((bm[b1 >> 5] >> (b1 & 31)) & 1)) return false;
  return ((bm[b2 >> 5] >> (b2 & 31)) & 1) != 0;
}

__device__ inline bool bloomMayHave(const JoinAggDesc& d, uint64_t key) {
  if (d.bloomLog2 == 0) return true;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloomLog2) - 1;
  uint32_t b1 = (uint32_t)h & mask;
  uint32_t b2 = (uint32_t)(h >> 32) & mask;
  auto bm = gptr<uint32_t>(d.bloom);  // AS1: keep probes off the flat path
  if (!((bm[b1 >> 5] >> (b1 & 31)) & 1)) return false;
  return ((bm[b2 >> 5] >> (b2 & 31)) & 1) != 0;
}

// count rows of build0 passing its predicate
// extra filter conjuncts beyond the specialized first one (VectorizedFilter
// CNF semantics: every conjunct must pass; NULL rejects)
__device__ inline bool jaExtraPreds(const DevTable& t, const PredDesc* px,
                                    int n, const uint8_t* sc, int scLen,
                                    int64_t row) {
  for (int j = 0; j < n; j++)
    if (!evalSimplePred(t, px[j], sc, scLen, row)) return false;
  return true;
}

// order-preserving u64 projection of the (non-negative) 128-bit accumulator
// for the radix-threshold top-N; exact candidates compact with the full
// 128-bit value and the host sorts them exactly
__device__ inline uint64_t jaKey64(const JoinAggDesc& d, int64_t i) {
  unsigned __int128 a =
      ((unsigned __int128)(uint64_t)gptr<int64_t>(&d.slots[i].accHi)[0] << 64) |
      gptr<uint64_t>(&d.slots[i].accLo)[0];
  return (uint64_t)(a >> d.topnShift);
}

__global__ void jaCountBuild0Kernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build0.nRows;
  uint64_t my = 0;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPred0 == 0 ||
                evalSimplePred(d.build0, d.pred0, d.strConst, d.strConstLen, row);
    if (pass && d.nPred0x)
      pass = jaExtraPreds(d.build0, d.pred0x, d.nPred0x, d.strConst,
                          d.strConstLen, row);
    if (pass) my++;
  }
  for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
  if ((threadIdx.x & 63) == 0 && my)
    atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
}

// insert passing build0 keys into the open-addressed key set
__global__ void jaBuild0Kernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build0.nRows;
  uint32_t mask = (1u << d.keySetLog2) - 1;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPred0 == 0 ||
                evalSimplePred(d.build0, d.pred0, d.strConst, d.strConstLen, row);
    if (pass && d.nPred0x)
      pass = jaExtraPreds(d.build0, d.pred0x, d.nPred0x, d.strConst,
                          d.strConstLen, row);
    if (!pass) continue;
    if (colIsNull(d.build0.cols[d.b0KeyCol], row)) continue;  // NULL never joins
    uint64_t key = gptr<uint64_t>(d.build0.cols[d.b0KeyCol].data)[row];
    if (key == kEmptyKey) key = kEmptyKey - 1;
    bloom0Set(d, key);
    uint32_t slot = (uint32_t)(hashKey(key) & mask);
    for (uint32_t probe = 0; probe <= mask; probe++) {
      uint64_t cur = d.keySet[slot];
      if (cur == key) break;
      if (cur == kEmptyKey) {
        uint64_t prev = atomicCAS((unsigned long long*)&d.keySet[slot],
                                  (unsigned long long)kEmptyKey,
                                  (unsigned long long)key);
        if (prev == kEmptyKey || prev == key) break;
      }
      slot = (slot + 1) & mask;
      if (probe == mask) atomicOr(d.errorFlag, kErrGlobalFull);
    }
  }
}

__device__ inline bool keySetHas(const JoinAggDesc& d, uint64_t key) {
  uint32_t mask = (1u << d.keySetLog2) - 1;
  if (key == kEmptyKey) key = kEmptyKey - 1;
  uint32_t slot = (uint32_t)(hashKey(key) & mask);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    uint64_t cur = gptr<uint64_t>(d.keySet)[slot];
    if (cur == key) return true;
    if (cur == kEmptyKey) return false;
    slot = (slot + 1) & mask;
  }
  return false;
}

// count build1 rows passing pred AND matching the key set
__global__ void jaCountBuild1Kernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build1.nRows;
  uint64_t my = 0;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPred1 == 0 ||
                evalSimplePred(d.build1, d.pred1, d.strConst, d.strConstLen, row);
    if (pass && d.nPred1x)
      pass = jaExtraPreds(d.build1, d.pred1x, d.nPred1x, d.strConst,
                          d.strConstLen, row);
    if (!pass) continue;
    const DevCol& kc = d.build1.cols[d.b1ProbeCol];
    if (colIsNull(kc, row)) continue;
    uint64_t pkey0 = gptr<uint64_t>(kc.data)[row];
    if (!bloom0MayHave(d, pkey0)) continue;  // L2-resident reject
    if (!keySetHas(d, pkey0)) continue;
    my++;
  }
  for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
  if ((threadIdx.x & 63) == 0 && my)
    atomicAdd((unsigned long long*)&d.counters[1], (unsigned long long)my);
}

// build the slot table from qualifying build1 rows
template <bool CHAIN = false>
__global__ void jaBuild1Kernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build1.nRows;
  uint32_t mask = (1u << d.slotsLog2) - 1;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPred1 == 0 ||
                evalSimplePred(d.build1, d.pred1, d.strConst, d.strConstLen, row);
    if (pass && d.nPred1x)
      pass = jaExtraPreds(d.build1, d.pred1x, d.nPred1x, d.strConst,
                          d.strConstLen, row);
    if (!pass) continue;
    const DevCol& pc = d.build1.cols[d.b1ProbeCol];
    if (colIsNull(pc, row)) continue;
    uint64_t pkey0 = gptr<uint64_t>(pc.data)[row];
    if (!bloom0MayHave(d, pkey0)) continue;  // L2-resident reject
    if (!keySetHas(d, pkey0)) continue;
    const DevCol& kc = d.build1.cols[d.b1KeyCol];
    if (colIsNull(kc, row)) continue;
    uint64_t key = gptr<uint64_t>(kc.data)[row];
    if (key == kEmptyKey) key = kEmptyKey - 1;
    uint64_t pay0 = d.payloadCol0 >= 0
        ? gptr<uint64_t>(d.build1.cols[d.payloadCol0].data)[row] : 0;
    int64_t pay1 = d.payloadCol1 >= 0
        ? gptr<int64_t>(d.build1.cols[d.payloadCol1].data)[row] : 0;
    bloomSet(d, key);
    if (CHAIN) {
      // duplicate-key mode: one slot PER BUILD1 ROW (each (key, payloads)
      // row is its own group), chained from the pow2 heads table like the
      // standalone join (hash_table_v2.go chains)
      JoinAggSlot& sp2 = d.slots[row];
      sp2.key = key;
      sp2.payload0 = pay0;
      sp2.payload1 = pay1;
      uint32_t hmask = (1u << d.b1HeadsLog2) - 1;
      uint32_t hslot = (uint32_t)(hashKey(key) & hmask);
      uint32_t newHead = (uint32_t)row + 1;
      uint32_t old = d.b1Heads[hslot];
      for (;;) {
        d.b1Next[row] = old;
        uint32_t prev = atomicCAS(&d.b1Heads[hslot], old, newHead);
        if (prev == old) break;
        old = prev;
      }
      continue;
    }
    uint32_t slot = (uint32_t)(hashKey(key) & mask);
    for (uint32_t probe = 0; probe <= mask; probe++) {
      uint64_t cur = d.slots[slot].key;
      if (cur == key) {
        // duplicate build key: the engine retries with the chained variant
        atomicOr(d.errorFlag, kErrBadKey);
        break;
      }
      if (cur == kEmptyKey) {
        uint64_t prev = atomicCAS((unsigned long long*)&d.slots[slot].key,
                                  (unsigned long long)kEmptyKey,
                                  (unsigned long long)key);
        if (prev == kEmptyKey) {
          d.slots[slot].payload0 = pay0;
          d.slots[slot].payload1 = pay1;
          break;
        }
        if (prev == key) { atomicOr(d.errorFlag, kErrBadKey); break; }
      }
      slot = (slot + 1) & mask;
      if (probe == mask) atomicOr(d.errorFlag, kErrGlobalFull);
    }
  }
}

// probe: scan the probe table; pred -> VM value -> probe slots -> accumulate.
// Payload writes may race with probe reads only via the key CAS (published
// before probing starts: build and probe are separate kernel launches, so
// visibility comes from the dispatch boundary, not intra-kernel hand-off).
template <bool WIDE, bool CHAIN = false>
__launch_bounds__(256)
__global__ void jaProbeKernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.probe.nRows;
  uint32_t mask = (1u << d.slotsLog2) - 1;
  int64_t per = (n + gridDim.x - 1) / gridDim.x;
  int64_t begin = (int64_t)blockIdx.x * per;
  int64_t end = begin + per;
  if (end > n) end = n;
  bool failed = false;
  uint64_t myMatch = 0;
  for (int64_t row = begin + threadIdx.x; row < end && !failed;
       row += blockDim.x) {
    RawState raw;
    fetchRow(d.probe, d.fetch, d.nFetch, row, raw);
    // predicate (slot-fetched when planned)
    bool pass = d.nPredP == 0;
    if (!pass) {
      const PredDesc& pd = d.predP;
      const DevCol& c = d.probe.cols[pd.col];
      if (colIsNull(c, row)) pass = false;
      else if (pd.kind == PRED_TIME_CMP_CONST) {
        uint64_t v = (pd.slot >= 0 ? raw.get(pd.slot).x
                                   : gptr<uint64_t>(c.data)[row]) & ~0xFULL;
        uint64_t k = pd.constU64 & ~0xFULL;
        pass = cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
      } else if (pd.kind == PRED_I64_CMP_CONST) {
        int64_t v = pd.slot >= 0 ? (int64_t)raw.get(pd.slot).x
                                 : gptr<int64_t>(c.data)[row];
        int64_t k = (int64_t)pd.constU64;
        pass = cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
      } else {
        pass = evalSimplePred(d.probe, pd, d.strConst, d.strConstLen, row);
      }
    }
    if (pass && d.nPredPx)
      pass = jaExtraPreds(d.probe, d.predPx, d.nPredPx, d.strConst,
                          d.strConstLen, row);
    if (!pass) continue;
    const DevCol& kc = d.probe.cols[d.pKeyCol];
    if (colIsNull(kc, row)) continue;
    uint64_t key = gptr<uint64_t>(kc.data)[row];
    if (key == kEmptyKey) key = kEmptyKey - 1;
    if (!bloomMayHave(d, key)) continue;  // L2-resident reject
    // probe the slot table (prebuilt: no inserts, miss -> drop row)
    uint32_t slot = 0;
    uint32_t firstCur = 0;
    if (CHAIN) {
      uint32_t hmask = (1u << d.b1HeadsLog2) - 1;
      uint32_t cur = gptr<uint32_t>(d.b1Heads)[(uint32_t)(hashKey(key) & hmask)];
      while (cur != 0) {
        if (gptr<uint64_t>(&d.slots[cur - 1].key)[0] == key) {
          firstCur = cur;
          break;
        }
        cur = gptr<uint32_t>(d.b1Next)[cur - 1];
      }
      if (firstCur == 0) continue;
    } else {
      slot = (uint32_t)(hashKey(key) & mask);
      bool found = false;
      for (uint32_t probe = 0; probe <= mask; probe++) {
        uint64_t cur = gptr<uint64_t>(&d.slots[slot].key)[0];
        if (cur == key) { found = true; break; }
        if (cur == kEmptyKey) break;
        slot = (slot + 1) & mask;
      }
      if (!found) continue;
    }
    // VM: compute the summed value
    VmState<WIDE> vm;
    vm.nullBits = 0;
    bool bad = false;
    bool ovf = false;
    for (int i = 0; i < d.nIns && !bad; i++) {
      const VmIns& ins = d.ins[i];
      switch (ins.op) {
        case VM_LOAD_DEC: {
          // lazy: only filter-surviving, join-matching rows reach the VM, so
          // value columns are loaded here (~5-10% of rows), not prefetched
          const DevCol& c = d.probe.cols[ins.a];
          bool nul = colIsNull(c, row);
          typename VT<WIDE>::T v = VT<WIDE>::zero();
          if (!nul && c.units) {
            // proven column: units at the declared frac (= ins.b)
            v = VT<WIDE>::fromI64(loadUnits(c, row), nullptr);
          } else if (!nul) {
            int sc;
            bool okp = ins.c >= 0
                ? parseDecimalRaw<WIDE>(raw.get(ins.c), &v, &sc, d.errorFlag)
                : loadDecimalUnits<WIDE>((const uint8_t*)c.data + row * 40, &v,
                                         &sc, d.errorFlag);
            if (!okp) {
              bad = true;
              break;
            }
            if (sc != ins.b) {
              if (sc < ins.b) v = VT<WIDE>::scale10(v, ins.b - sc, &ovf);
              else { atomicOr(d.errorFlag, kErrScale); bad = true; break; }
            }
          }
          vm.set(ins.dst, v);
          vm.setNull(ins.dst, nul);
          break;
        }
        case VM_LOAD_I64: {
          const DevCol& c = d.probe.cols[ins.a];
          bool nul = colIsNull(c, row);
          int64_t lv = 0;
          if (!nul)
            lv = ins.c >= 0 ? (int64_t)raw.get(ins.c).x
                            : ((const int64_t*)c.data)[row];
          vm.set(ins.dst, nul ? VT<WIDE>::zero() : VT<WIDE>::fromI64(lv, &ovf));
          vm.setNull(ins.dst, nul);
          break;
        }
        default:
          if (!vmStep<WIDE, kVmOpsCore>(vm, ins, d.insP10[i], d.constLo,
                                        d.constHi, d.errorFlag, &ovf))
            bad = true;
          break;
      }
    }
    if (ovf) {
      atomicOr(d.errorFlag, WIDE ? kErrOverflow : kErrRetryWide);
      failed = true;
      break;
    }
    if (bad) { failed = true; break; }
    if (vm.isNull(d.valueReg)) continue;  // NULL never enters the sum
    Int128 v = VT<WIDE>::toAcc(vm.get(d.valueReg));
    if (CHAIN) {
      // every duplicate build row with this key is its own group: the probe
      // row's value accumulates into each (one pair per build row)
      for (uint32_t cur = firstCur; cur != 0;
           cur = gptr<uint32_t>(d.b1Next)[cur - 1]) {
        uint32_t brow = cur - 1;
        if (gptr<uint64_t>(&d.slots[brow].key)[0] != key) continue;
        JoinAggSlot* sp = &d.slots[brow];
        uint64_t old = atomicAdd((unsigned long long*)&sp->accLo,
                                 (unsigned long long)v.lo);
        uint64_t carry = (old + v.lo) < old ? 1 : 0;
        int64_t hiAdd = v.hi + (int64_t)carry;
        if (hiAdd != 0)
          atomicAdd((unsigned long long*)&sp->accHi,
                    (unsigned long long)hiAdd);
        if (v.hi < 0 || (v.hi == 0 && v.lo == 0))
          atomicAdd((unsigned long long*)&sp->cnt, 1ULL);
        myMatch++;
      }
      continue;
    }
    JoinAggSlot* sp = &d.slots[slot];
    uint64_t old = atomicAdd((unsigned long long*)&sp->accLo, (unsigned long long)v.lo);
    uint64_t carry = (old + v.lo) < old ? 1 : 0;
    int64_t hiAdd = v.hi + (int64_t)carry;
    if (hiAdd != 0)
      atomicAdd((unsigned long long*)&sp->accHi, (unsigned long long)hiAdd);
    // the count atomic exists to mark the group matched; a contribution > 0
    // already proves that through acc (sums can only return to zero if some
    // contribution was <= 0, and those always count) -> one atomic per match
    // on all-positive data
    if (v.hi < 0 || (v.hi == 0 && v.lo == 0))
      atomicAdd((unsigned long long*)&sp->cnt, 1ULL);
    myMatch++;
  }
  for (int off = 32; off > 0; off >>= 1) myMatch += __shfl_down(myMatch, off, 64);
  if ((threadIdx.x & 63) == 0 && myMatch)
    atomicAdd((unsigned long long*)&d.counters[2], (unsigned long long)myMatch);
}

// top-N selection: pass A finds the max ACC HI WORD (and flags negative
// accumulators — the order-preserving shift projection needs non-negative
// revenues; Q3's price*(1-disc) always is); the engine derives topnShift so
// key64 = acc128 >> shift fits u64; pass B (jaMaxKernel) then maxes key64.
// chained mode: duplicate build1 rows with IDENTICAL (key, payloads) are
// ONE group in the reference (each probe row matched both, so the sums
// add); merge every such slot into the chain-first canonical slot. Only the
// owning thread reads/clears its own slot; everyone adds into canonicals.
__global__ void jaMergeDupSlotsKernel(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.nSlots;
  uint32_t hmask = (1u << d.b1HeadsLog2) - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t key = gptr<uint64_t>(&d.slots[i].key)[0];
    if (key == kEmptyKey) continue;
    uint64_t p0 = gptr<uint64_t>(&d.slots[i].payload0)[0];
    int64_t p1 = gptr<int64_t>(&d.slots[i].payload1)[0];
    uint32_t canon = 0;
    for (uint32_t cur =
             gptr<uint32_t>(d.b1Heads)[(uint32_t)(hashKey(key) & hmask)];
         cur != 0; cur = gptr<uint32_t>(d.b1Next)[cur - 1]) {
      uint32_t r = cur - 1;
      if (gptr<uint64_t>(&d.slots[r].key)[0] == key &&
          gptr<uint64_t>(&d.slots[r].payload0)[0] == p0 &&
          gptr<int64_t>(&d.slots[r].payload1)[0] == p1) {
        canon = cur;
        break;
      }
    }
    if (canon == 0 || (int64_t)(canon - 1) == i) continue;
    JoinAggSlot* dst = &d.slots[canon - 1];
    const JoinAggSlot& s = d.slots[i];
    uint64_t old = atomicAdd((unsigned long long*)&dst->accLo,
                             (unsigned long long)s.accLo);
    uint64_t carry = (old + s.accLo) < old ? 1 : 0;
    int64_t hiAdd = s.accHi + (int64_t)carry;
    if (hiAdd != 0)
      atomicAdd((unsigned long long*)&dst->accHi, (unsigned long long)hiAdd);
    if (s.cnt)
      atomicAdd((unsigned long long*)&dst->cnt, (unsigned long long)s.cnt);
    d.slots[i].key = kEmptyKey;  // only this thread touches slot i
  }
}

__global__ void jaMaxHiKernel(const JoinAggDesc* __restrict__ dp,
                              uint64_t* outMaxHi) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.nSlots;
  uint64_t my = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t skey = gptr<uint64_t>(&d.slots[i].key)[0];
    if (skey == kEmptyKey) continue;
    int64_t hi = gptr<int64_t>(&d.slots[i].accHi)[0];
    if (hi < 0) atomicOr(d.errorFlag, kErrOverflow);  // negative revenue
    if ((uint64_t)hi > my) my = (uint64_t)hi;
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o = __shfl_down(my, off, 64);
    if (o > my) my = o;
  }
  if ((threadIdx.x & 63) == 0) atomicMax((unsigned long long*)outMaxHi, my);
}

__global__ void jaMaxKernel(const JoinAggDesc* __restrict__ dp, uint64_t* outMax) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.nSlots;
  uint64_t my = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t skey = gptr<uint64_t>(&d.slots[i].key)[0];
    if (skey == kEmptyKey) continue;
    if (gptr<uint64_t>(&d.slots[i].accLo)[0] == 0 &&
        gptr<uint64_t>(&d.slots[i].accHi)[0] == 0 &&
        gptr<uint64_t>(&d.slots[i].cnt)[0] == 0)
      continue;
    uint64_t k64 = jaKey64(d, i);
    if (k64 > my) my = k64;
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o = __shfl_down(my, off, 64);
    if (o > my) my = o;
  }
  if ((threadIdx.x & 63) == 0) atomicMax((unsigned long long*)outMax, my);
}

__global__ void jaHistKernel(const JoinAggDesc* __restrict__ dp, uint32_t* hist,
                             int shift) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.nSlots;
  // ~14M occupied slots funneling into 4096 bins: privatize the histogram
  // in LDS per block and flush once (the global-atomic version measured
  // 6.4 ms of pure contention, 25x the scan floor)
  __shared__ uint32_t lh[4096];
  for (int b = threadIdx.x; b < 4096; b += blockDim.x) lh[b] = 0;
  __syncthreads();
  auto lh3 = (__attribute__((address_space(3))) uint32_t*)lh;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t key = gptr<uint64_t>(&d.slots[i].key)[0];
    if (key == kEmptyKey) continue;
    uint64_t accLo = gptr<uint64_t>(&d.slots[i].accLo)[0];
    if (accLo == 0 && gptr<uint64_t>(&d.slots[i].accHi)[0] == 0 &&
        gptr<uint64_t>(&d.slots[i].cnt)[0] == 0)
      continue;
    __hip_atomic_fetch_add(&lh3[(jaKey64(d, i) >> shift) & 4095], 1u,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 4096; b += blockDim.x)
    if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

__global__ void jaCompactKernel(const JoinAggDesc* __restrict__ dp, TopNOut* out,
                                uint64_t* outCount, uint64_t thresholdBucket,
                                int shift, uint64_t cap) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.nSlots;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t skey = gptr<uint64_t>(&d.slots[i].key)[0];
    if (skey == kEmptyKey) continue;
    const JoinAggSlot& s = d.slots[i];
    if (s.cnt == 0 && s.accLo == 0 && s.accHi == 0) continue;
    if ((jaKey64(d, i) >> shift) < thresholdBucket) continue;
    uint64_t idx = atomicAdd((unsigned long long*)outCount, 1ULL);
    if (idx >= cap) { atomicOr(d.errorFlag, kErrGlobalFull); continue; }
    out[idx] = {s.key, s.payload0, s.payload1, s.accLo, s.accHi};
  }
}

// ==================================================================
// glds-staged fused aggregation
// ==================================================================
// Per-wave double-buffered tile pipeline: each wave owns tiles of 64 rows;
// all streams of tile t+1 are DMA'd HBM->LDS (`global_load_lds`, no VGPR
// round-trip) while tile t is consumed from LDS (parse + VM + aggregate).
// Counted `s_waitcnt vmcnt(N)` keeps the next tile's DMAs in flight across
// the compute (guide §5 'Pipelining across barriers'); all LDS lives in ONE
// dynamic __shared__ carve (a second __shared__ object would make hipcc
// drain vmcnt before every ds_read — guide §5 'Three .s-level traps').

typedef __attribute__((address_space(3))) char LdsChar;
typedef __attribute__((address_space(3))) GroupSlot LdsGroupSlot;

// LDS-table accumulate via explicit AS3 atomics (generic-pointer HIP atomics
// lower to flat ops, which count on vmcnt and would break the counted-wait
// DMA pipeline)
__device__ inline void accumIntoLds(LdsGroupSlot* slot, int a, Int128 v,
                                    int64_t dc) {
  if (v.lo != 0 || v.hi != 0) {
    uint64_t old = __hip_atomic_fetch_add(&slot->accLo[a], (uint64_t)v.lo,
                                          __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
    uint64_t carry = (old + v.lo) < old ? 1 : 0;
    int64_t hiAdd = v.hi + (int64_t)carry;
    if (hiAdd != 0)
      __hip_atomic_fetch_add((__attribute__((address_space(3)))uint64_t*)&slot->accHi[a], (uint64_t)hiAdd,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (dc != 0)
    __hip_atomic_fetch_add((__attribute__((address_space(3)))uint64_t*)&slot->cnt[a], (uint64_t)dc,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ inline void gldsWaitVmcnt(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
  }
}

// issue all stream DMAs for one 64-row tile into tileBuf (wave-uniform base)
__device__ __attribute__((always_inline)) inline void gldsIssueTile(
    const FusedQueryDesc& d, int64_t row0, int64_t clampMax, LdsChar* tileBuf,
    int lane) {
  for (int f0 = 0; f0 < d.nFetch; f0++) {
    int f = __builtin_amdgcn_readfirstlane(f0);  // uniform -> scalar desc loads
    const FetchDesc& fd = d.fetch[f];
    const DevCol& c = d.table.cols[__builtin_amdgcn_readfirstlane(fd.col)];
    auto lptr = (__attribute__((address_space(3))) void*)(tileBuf + fd.ldsOff);
    if (fd.kind == FETCH_DEC16) {
      int64_t r = row0 + lane;
      if (r > clampMax) r = clampMax;  // tail rows re-read the last row
      auto g = (const __attribute__((address_space(1))) void*)
          ((const uint8_t*)c.data + r * 40);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) uint32_t*)g,
          (__attribute__((address_space(3))) uint32_t*)lptr, 16, 0, 0);
    } else if (fd.kind == FETCH_8B) {
      if (lane < 32) {
        int64_t r = row0 + 2 * lane;
        if (r > clampMax) r = clampMax;
        auto g = (const __attribute__((address_space(1))) void*)
            ((const uint8_t*)c.data + r * 8);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) uint32_t*)g,
            (__attribute__((address_space(3))) uint32_t*)lptr, 16, 0, 0);
      }
    } else {  // FETCH_B1
      if (lane < 16) {
        int64_t r = row0 + 4 * lane;
        if (r > clampMax - 3) r = clampMax - 3 < 0 ? 0 : clampMax - 3;
        auto g = (const __attribute__((address_space(1))) void*)
            ((const uint8_t*)c.data + r);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) uint32_t*)g,
            (__attribute__((address_space(3))) uint32_t*)lptr, 4, 0, 0);
      }
    }
  }
}

// LDS-backed raw accessor for one row (lane) of the staged tile. The buffer
// pointer is LDS-qualified so reads lower to ds_read (a generic pointer
// would emit flat loads, which count on vmcnt and break the pipeline).
struct LdsRaw {
  const LdsChar* buf;
  const FusedQueryDesc* d;  // LDS-resident copy (see kernel prologue)
  int lane;
  __device__ ulonglong2 get(int slot) const {
    const FetchDesc& fd = d->fetch[__builtin_amdgcn_readfirstlane(slot)];
    if (fd.kind == FETCH_DEC16) {
      auto p = (const __attribute__((address_space(3))) uint64_t*)(buf + fd.ldsOff + lane * 16);
      ulonglong2 v;
      v.x = p[0];
      v.y = p[1];
      return v;
    }
    if (fd.kind == FETCH_8B) {
      ulonglong2 v;
      v.x = *(const __attribute__((address_space(3))) uint64_t*)(buf + fd.ldsOff + lane * 8);
      v.y = 0;
      return v;
    }
    ulonglong2 v;
    v.x = *(const __attribute__((address_space(3))) uint8_t*)(buf + fd.ldsOff + lane);
    v.y = 0;
    return v;
  }
};

// group key from staged streams (dense-char via B1 slot, i64 via 8B slot)
template <typename RAW>
__device__ inline bool makeGroupKeyStaged(const FusedQueryDesc& d,
                                          const RAW& raw, uint64_t* keyOut,
                                          uint32_t* err) {
  uint64_t key = 0;
  for (int k0 = 0; k0 < d.gkey.nCols; k0++) {
    int k = __builtin_amdgcn_readfirstlane(k0);
    uint32_t lane32;
    if (d.gkey.kind[k] == 2) {
      uint8_t b = (uint8_t)raw.get(d.gkey.slot[k]).x;
      lane32 = b == ' ' ? 0u : ((1u << 24) | b);
    } else {  // kind 1: small i64
      int64_t v = (int64_t)raw.get(d.gkey.slot[k]).x;
      if (v < 0 || v > 0x7FFFFFFF) { atomicOr(err, kErrBadKey); return false; }
      lane32 = (uint32_t)v;
    }
    key |= (uint64_t)lane32 << (32 * k);
  }
  if (d.gkey.nCols == 0) key = 0;
  if (key == kEmptyKey) key = kEmptyKey - 1;
  *keyOut = key;
  return true;
}

// row pipeline over a staged tile row (mirrors processRow; RAW = LdsRaw)
template <bool WIDE>
__device__ __attribute__((always_inline)) inline bool processRowStaged(
    const FusedQueryDesc& d, const LdsRaw& raw, LdsGroupSlot* lds,
    uint64_t* mySel) {
  bool pass = true;
  for (int p0 = 0; p0 < d.nPreds && pass; p0++) {
    const PredDesc& pd = d.preds[__builtin_amdgcn_readfirstlane(p0)];
    if (pd.kind == PRED_TIME_CMP_CONST) {
      uint64_t v = raw.get(pd.slot).x & ~0xFULL;
      uint64_t k = pd.constU64 & ~0xFULL;
      pass = cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
    } else if (pd.kind == PRED_I64_CMP_CONST) {
      int64_t v = (int64_t)raw.get(pd.slot).x;
      int64_t k = (int64_t)pd.constU64;
      pass = cmpResult(v < k ? -1 : (v > k ? 1 : 0), pd.cmp);
    } else {  // decimal pred via its DEC16 slot
      typename VT<WIDE>::T u;
      int sc;
      if (!parseDecimalRaw<WIDE>(raw.get(pd.slot), &u, &sc, d.errorFlag))
        return false;
      int cmp = VT<WIDE>::cmp(u, VT<WIDE>::fromI64((int64_t)pd.constU64, nullptr));
      pass = cmpResult(cmp, pd.cmp);
    }
  }
  if (!pass) return true;
  (*mySel)++;

  VmState<WIDE> vm;
  vm.nullBits = 0;
  bool bad = false;
  bool ovf = false;
  for (int i0 = 0; i0 < d.nIns && !bad; i0++) {
    const VmIns& ins = d.ins[__builtin_amdgcn_readfirstlane(i0)];
    switch (ins.op) {
      case VM_LOAD_DEC: {
        typename VT<WIDE>::T v = VT<WIDE>::zero();
        int sc;
        if (!parseDecimalRaw<WIDE>(raw.get(ins.c), &v, &sc, d.errorFlag,
                                   ins.b, d.insP10[i0], d.insMagic[i0])) {
          bad = true;
          break;
        }
        if (sc != ins.b) {
          if (sc < ins.b) v = VT<WIDE>::scale10(v, ins.b - sc, &ovf);
          else { atomicOr(d.errorFlag, kErrScale); bad = true; break; }
        }
        vm.set(ins.dst, v);
        vm.setNull(ins.dst, false);
        break;
      }
      case VM_LOAD_I64:
        vm.set(ins.dst, VT<WIDE>::fromI64((int64_t)raw.get(ins.c).x, &ovf));
        vm.setNull(ins.dst, false);
        break;
      default:
        if (!vmStep<WIDE, kVmOpsCore>(vm, ins, d.insP10[i0], d.constLo,
                                      d.constHi, d.errorFlag, &ovf))
          bad = true;
        break;
    }
  }
  if (ovf) {
    atomicOr(d.errorFlag, WIDE ? kErrOverflow : kErrRetryWide);
    return false;
  }
  if (bad) return false;
  if (d.ablate == 1) {
    uint64_t sink = 0;
    for (int a = 0; a < d.nAggs; a++)
      if (d.aggs[a].srcReg >= 0)
        sink ^= (uint64_t)VT<WIDE>::toAcc(vm.get(d.aggs[a].srcReg)).lo;
    asm volatile("" ::"v"(sink));
    return true;
  }

  uint64_t key;
  if (!makeGroupKeyStaged(d, raw, &key, d.errorFlag)) return false;
  // (the glds variant always uses the LDS table; the engine runs the plain
  // kernel for the high-NDV global-direct retry)
  uint32_t slot = (uint32_t)(splitmix64(key) & (kLdsGroups - 1));
  for (int probe = 0;; probe++) {
    if (probe >= kLdsGroups) { atomicOr(d.errorFlag, kErrLdsFull); return false; }
    uint64_t cur = lds[slot].key;
    if (cur == key) break;
    if (cur == kEmptyKey) {
      uint64_t expected = kEmptyKey;
      bool won = __hip_atomic_compare_exchange_strong(
          &lds[slot].key, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_WORKGROUP);
      if (won || expected == key) break;
    }
    slot = (slot + 1) & (kLdsGroups - 1);
  }
  LdsGroupSlot* target = &lds[slot];
  if (d.sharedCnt) accumIntoLds(target, 0, Int128{0, 0}, 1);
  for (int s0 = 0; s0 < d.nAccSlots; s0++) {
    int s = __builtin_amdgcn_readfirstlane(s0);
    int reg = d.accReg[s];
    accumIntoLds(target, s, VT<WIDE>::toAcc(vm.get(reg)), 0);
  }
  if (!d.sharedCnt) {
    for (int a0 = 0; a0 < d.nAggs; a0++) {
      int a = __builtin_amdgcn_readfirstlane(a0);
      if (d.aggs[a].fr >= 0) continue;
      accumIntoLds(target, a, Int128{0, 0}, 1);
    }
  }
  return true;
}

template <bool WIDE>
__launch_bounds__(256)
__global__ void fusedAggGldsKernel(const FusedQueryDesc* __restrict__ dp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr size_t kTableBytes = (sizeof(GroupSlot) * kLdsGroups + 15) & ~15ULL;
  auto lds = (LdsGroupSlot*)(LdsChar*)smem;
  auto tilesBase = (LdsChar*)smem + kTableBytes;
  for (int i = threadIdx.x; i < kLdsGroups; i += blockDim.x) {
    lds[i].key = kEmptyKey;
    for (int a = 0; a < kMaxAggs; a++) {
      lds[i].accLo[a] = 0;
      lds[i].accHi[a] = 0;
      lds[i].cnt[a] = 0;
    }
  }
  __syncthreads();
  const FusedQueryDesc& d = *dp;

  int64_t n = d.table.nRows;
  int64_t per = ((n + gridDim.x - 1) / gridDim.x + 63) & ~63LL;
  int64_t begin = (int64_t)blockIdx.x * per;
  int64_t end = begin + per;
  if (end > n) end = n;
  int wave = threadIdx.x >> 6;
  int lane = threadIdx.x & 63;
  LdsChar* myTiles = tilesBase + (size_t)wave * 2 * d.tileBytes;
  uint64_t mySel = 0;
  bool failed = false;

  // tiles of 64 rows, strided across the block's 4 waves
  int64_t range = end - begin;
  int64_t nTiles = (range + 63) / 64;
  int64_t t = wave;
  if (t < nTiles)
    gldsIssueTile(d, begin + t * 64, end - 1, myTiles, lane);
  int buf = 0;
  for (; t < nTiles && !failed; t += 4) {
    int64_t nextT = t + 4;
    bool haveNext = nextT < nTiles;
    if (haveNext)
      gldsIssueTile(d, begin + nextT * 64, end - 1, myTiles + (buf ^ 1) * d.tileBytes,
                    lane);
    // wait for tile t's DMAs (the next tile's stay in flight)
    gldsWaitVmcnt(haveNext ? d.nFetch : 0);
    int64_t row = begin + t * 64 + lane;
    if (row < end) {
      LdsRaw raw{myTiles + buf * d.tileBytes, &d, lane};
      if (!processRowStaged<WIDE>(d, raw, lds, &mySel)) failed = true;
    }
    buf ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if (d.selCount) {
    uint64_t total = mySel;
    for (int off = 32; off > 0; off >>= 1)
      total += __shfl_down(total, off, 64);
    if ((threadIdx.x & 63) == 0 && total)
      atomicAdd((unsigned long long*)d.selCount, (unsigned long long)total);
  }
  __syncthreads();

  for (int i = threadIdx.x; i < kLdsGroups; i += blockDim.x) {
    if (lds[i].key == kEmptyKey) continue;
    uint64_t key = lds[i].key;
    uint32_t gmask = (1u << d.globalGroupsLog2) - 1;
    uint32_t slot = (uint32_t)(splitmix64(key) & gmask);
    bool ok = true;
    for (uint32_t probe = 0;; probe++) {
      if (probe > gmask) { atomicOr(d.errorFlag, kErrGlobalFull); ok = false; break; }
      uint64_t cur = d.globalTable[slot].key;
      if (cur == key) break;
      if (cur == kEmptyKey) {
        uint64_t prev = atomicCAS((unsigned long long*)&d.globalTable[slot].key,
                                  (unsigned long long)kEmptyKey,
                                  (unsigned long long)key);
        if (prev == kEmptyKey || prev == key) break;
      }
      slot = (slot + 1) & gmask;
    }
    if (!ok) continue;
    for (int s = 0; s < d.nAccSlots; s++) {
      if (d.accKind[s] != 0) {
        accumMax(&d.globalTable[slot], s, lds[i].accLo[s]);
        continue;
      }
      Int128 v = {lds[i].accLo[s], lds[i].accHi[s]};
      accumInto(&d.globalTable[slot], s, v, 0);
    }
    int nCnt = d.sharedCnt ? 1 : d.nAggs;
    for (int a = 0; a < nCnt; a++)
      accumInto(&d.globalTable[slot], a, Int128{0, 0}, lds[i].cnt[a]);
  }
}

__global__ void jaInitSlotsKernel(JoinAggSlot* slots, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  slots[i].key = kEmptyKey;
  slots[i].payload0 = 0;
  slots[i].payload1 = 0;
  slots[i].accLo = 0;
  slots[i].accHi = 0;
  slots[i].cnt = 0;
}

// ---- orders / customer generators ----
__global__ void genOrdersKernel(DevTable tab, int64_t rowBegin, int64_t nRows,
                                uint64_t seed, int64_t totalRows) {
  int64_t nCust = totalRows / 10;
  if (nCust < 1) nCust = 1;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nRows;
       i += stride) {
    int64_t row = rowBegin + i;
    ((int64_t*)tab.cols[0].data)[i] = row + 1;
    ((int64_t*)tab.cols[1].data)[i] =
        1 + (int64_t)(fieldRand(seed, row, 1) % (uint64_t)nCust);
    int y, m, dd;
    civilFromDays(GX_EPOCH_1992 +
                      (int64_t)(fieldRand(seed, row, 2) % (uint64_t)GX_ORDERDATE_DAYS),
                  &y, &m, &dd);
    ((uint64_t*)tab.cols[2].data)[i] = timeFromDate(y, m, dd);
    ((int64_t*)tab.cols[3].data)[i] = 0;
  }
}

__device__ __constant__ const char kSegChars[5][11] = {
    "AUTOMOBILE", "BUILDING", "FURNITURE", "MACHINERY", "HOUSEHOLD"};
__device__ __constant__ const int kSegLens[5] = {10, 8, 9, 9, 9};

__global__ void genCustomerLenKernel(int64_t* lens, int64_t rowBegin,
                                     int64_t nRows, uint64_t seed) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nRows;
       i += stride)
    lens[i] = kSegLens[fieldRand(seed, rowBegin + i, 1) % 5];
}

__global__ void genCustomerFillKernel(DevTable tab, int64_t rowBegin,
                                      int64_t nRows, uint64_t seed) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nRows;
       i += stride) {
    int64_t row = rowBegin + i;
    ((int64_t*)tab.cols[0].data)[i] = row + 1;
    int seg = (int)(fieldRand(seed, row, 1) % 5);
    int64_t off = tab.cols[1].offsets[i];
    for (int j = 0; j < kSegLens[seg]; j++)
      ((uint8_t*)tab.cols[1].data)[off + j] = kSegChars[seg][j];
  }
}

// ---------------- host launch wrappers ----------------

int gxLaunchTpchGen(int table, DevTable* devTab, int64_t rowBegin, int64_t nRows,
                    uint64_t seed, int64_t totalRows, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int block = 256;
  int grid = (int)((nRows + block - 1) / block);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  if (table == 0) {
    hipLaunchKernelGGL(genLineitemKernel, dim3(grid), dim3(block), 0, s, *devTab,
                       rowBegin, nRows, seed, totalRows);
  } else {
    return -1;  // orders/customer device generation lands with the Q3 path
  }
  return (int)hipGetLastError();
}

__global__ void dumpDescKernel(const FusedQueryDesc* dp) {
  if (threadIdx.x || blockIdx.x) return;
  const FusedQueryDesc& d = *dp;
  printf("[dev] nIns=%d nAggs=%d nAccSlots=%d sharedCnt=%d wide=%d\n",
         d.nIns, d.nAggs, d.nAccSlots, d.sharedCnt, d.wide);
  for (int i = 0; i < d.nIns; i++)
    printf("[dev] ins[%d] op=%d dst=%d a=%d b=%d c=%d p10=%lld\n", i,
           d.ins[i].op, d.ins[i].dst, d.ins[i].a, d.ins[i].b, d.ins[i].c,
           (long long)d.insP10[i]);
  for (int a = 0; a < d.nAggs; a++)
    printf("[dev] agg[%d] func=%d srcReg=%d scale=%d fr=%d accMap=%d\n", a,
           d.aggs[a].func, d.aggs[a].srcReg, d.aggs[a].scale, d.aggs[a].fr,
           d.accMap[a]);
  for (int s = 0; s < d.nAccSlots; s++)
    printf("[dev] accReg[%d]=%d\n", s, d.accReg[s]);
  printf("[dev] kP10(18)=%lld sizeof(desc)=%d aggs_off=%d ins_off=%d\n",
         (long long)kP10(18), (int)sizeof(FusedQueryDesc),
         (int)((char*)&d.aggs[0] - (char*)&d), (int)((char*)&d.ins[0] - (char*)&d));
}

int gxDumpDesc(const FusedQueryDesc* devDesc, void* stream) {
  hipLaunchKernelGGL(dumpDescKernel, dim3(1), dim3(1), 0, (hipStream_t)stream, devDesc);
  hipStreamSynchronize((hipStream_t)stream);
  return (int)hipGetLastError();
}

int gxFusedGrid(int64_t rows) {
  int grid = (int)((rows + 255) / 256);
  // >> 256 workgroups to fill 256 CUs / 8 XCDs; cap and grid-stride per block
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  return grid;
}

// ---- decimal units column (DevCol::units) ----
// One pass over a resident 40 B decimal column: the same two 8-byte loads as
// loadDecimalUnits, the same arithmetic as the narrow parseDecimalRaw, one
// coalesced 8 B store per lane. A row that is not exactly servable (bad
// header, digitsFrac != declaredFrac, units beyond int64) only raises the
// flag -- no error moves to bind time; the engine drops the buffer and the
// column keeps its FETCH_DEC16 path with every error surface where it was.
// flag[1] collects the width class the non-NULL units need (gx_units.h): a
// per-wave maximum, at most one atomic per wave.
__launch_bounds__(256)
__global__ void buildDecUnitsKernel(DevCol col, int64_t nRows, int declaredFrac,
                                    int64_t* __restrict__ out, uint32_t* flag) {
  const int64_t p10v = kP10(declaredFrac);
  const uint64_t magic = kDivMagic(9 - declaredFrac);
  bool bad = false;
  int wcls = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < nRows; row += stride) {
    int64_t units = 0;
    const bool nul = colIsNull(col, row);
    if (!nul) {
      const uint8_t* p = (const uint8_t*)col.data + row * 40;
      uint64_t w0 = *gptr<uint64_t>(p);
      uint64_t w1 = *gptr<uint64_t>(p + 8);
      uint32_t hdr = (uint32_t)w0;
      int digitsInt = (int)(int8_t)(hdr & 0xFF);
      int digitsFrac = (int)(int8_t)((hdr >> 8) & 0xFF);
      bool neg = ((hdr >> 24) & 0xFF) != 0;
      if (digitsInt < 0 || digitsInt > 18 || digitsFrac != declaredFrac) {
        bad = true;
      } else {
        int wordsInt = (digitsInt + 8) / 9;
        int32_t word0 = (int32_t)(uint32_t)(w0 >> 32);
        int32_t word1 = (int32_t)(uint32_t)w1;
        uint32_t word2 = (uint32_t)(w1 >> 32);
        int64_t ip = 0;
        if (wordsInt == 1) ip = word0;
        else if (wordsInt == 2) ip = (int64_t)word0 * 1000000000 + word1;
        uint32_t fw = wordsInt == 0 ? (uint32_t)word0
                                    : (wordsInt == 1 ? (uint32_t)word1 : word2);
        int64_t fr = declaredFrac > 0
                         ? (int64_t)(((unsigned __int128)fw * magic) >> 62)
                         : 0;
        bool ovf = __builtin_mul_overflow(ip, p10v, &units);
        ovf |= __builtin_add_overflow(units, fr, &units);
        if (ovf) { bad = true; units = 0; }
        else if (neg) units = -units;
      }
    }
    out[row] = units;
    if (!nul) {
      const int w = unitsWidthOf(units);
      if (w > wcls) wcls = w;
    }
  }
  // at most one atomic per failing wave
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
  // the classes are 1, 2, 4, 8: the wave's maximum is the top bit of their OR
  uint32_t wave = (uint32_t)wcls;
  for (int off = 32; off > 0; off >>= 1) wave |= __shfl_xor(wave, off, 64);
  if (wave && (threadIdx.x & 63) == 0)
    atomicMax(flag + 1, 1u << (31 - __clz(wave)));
}

// second bind-time pass of a units column whose proven range fits 1, 2 or
// 4 bytes: one 8 B load and one narrow store per row
__launch_bounds__(256)
__global__ void narrowUnitsKernel(const int64_t* __restrict__ in,
                                  int64_t nRows, int width, void* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < nRows; row += stride)
    unitsStore(out, width, row, gptr<int64_t>(in)[row]);
}

int gxBuildDecUnits(const DevCol& col, int64_t nRows, int declaredFrac,
                    int64_t* out, uint32_t* flag, void* stream) {
  if (declaredFrac < 0 || declaredFrac > 9) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(buildDecUnitsKernel, dim3(gxFusedGrid(nRows)), dim3(256),
                     0, (hipStream_t)stream, col, nRows, declaredFrac, out,
                     flag);
  return (int)hipGetLastError();
}

int gxNarrowUnits(const int64_t* in, int64_t nRows, int width, void* out,
                  void* stream) {
  if (width != 1 && width != 2 && width != 4) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(narrowUnitsKernel, dim3(gxFusedGrid(nRows)), dim3(256), 0,
                     (hipStream_t)stream, in, nRows, width, out);
  return (int)hipGetLastError();
}

int gxLaunchInitTable(GroupSlot* table, int64_t nSlots, void* stream) {
  hipLaunchKernelGGL(initGlobalTableKernel,
                     dim3((int)((nSlots + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, table, nSlots);
  return (int)hipGetLastError();
}

int gxLaunchCompactGroups(const FusedQueryDesc* devDesc, int globalGroupsLog2,
                          int usedBanks, FusedResultBlock* out, void* stream) {
  const int64_t nSlots1 = (int64_t)1 << globalGroupsLog2;
  hipLaunchKernelGGL(compactGroupsKernel, dim3((int)((nSlots1 + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, devDesc, usedBanks,
                     out);
  return (int)hipGetLastError();
}

int gxLaunchFusedAgg(const FusedQueryDesc& desc, const FusedQueryDesc* devDesc,
                     void* stream, int skipInit) {
  hipStream_t s = (hipStream_t)stream;
  int grid = gxFusedGrid(desc.table.nRows);
  // banks beyond 0 are written (and later read) only by a noLds pass
  int64_t nSlots = (int64_t)(1 << desc.globalGroupsLog2) *
                   (desc.noLds ? desc.accBanks : 1);
  if (!skipInit) {  // out-of-core slices accumulate into the SAME table
    hipLaunchKernelGGL(initGlobalTableKernel, dim3((int)((nSlots + 255) / 256)),
                       dim3(256), 0, s, desc.globalTable, nSlots);
    if (desc.gkey.wideMode && desc.gkey.recCursor)
      hipMemsetAsync(desc.gkey.recCursor, 0, 8, s);
  }
  if (desc.useGlds) {
    size_t shmem = ((sizeof(GroupSlot) * kLdsGroups + 15) & ~15ULL) +
                   (size_t)4 * 2 * desc.tileBytes;
    if (desc.wide)
      hipLaunchKernelGGL((fusedAggGldsKernel<true>), dim3(grid), dim3(256),
                         shmem, s, devDesc);
    else
      hipLaunchKernelGGL((fusedAggGldsKernel<false>), dim3(grid), dim3(256),
                         shmem, s, devDesc);
  } else if (desc.gkey.wideMode) {
    // serialized wide group keys: one general variant (R=8, div-capable,
    // 14-reg VM) x narrow/wide arithmetic
    if (desc.wide)
      hipLaunchKernelGGL((fusedAggKernel<true, 8, true, 14, true>), dim3(grid),
                         dim3(256), 0, s, devDesc);
    else
      hipLaunchKernelGGL((fusedAggKernel<false, 8, true, 14, true>), dim3(grid),
                         dim3(256), 0, s, devDesc);
  } else {
    // pick the 5-slot raw-state variant when every non-staged fetch slot
    // fits (higher occupancy for Q1-shaped queries)
    int maxSlot = -1;
    for (int f = 0; f < desc.nFetch; f++)
      if (desc.fetch[f].kind != FETCH_B1 && f > maxSlot) maxSlot = f;
    bool small = maxSlot < 5;
    if (desc.nVmRegs > 12) {
      // wide-projection plans: the 14-register VM state variant (R=8)
      if (desc.hasDiv) {
        if (desc.wide)
          hipLaunchKernelGGL((fusedAggKernel<true, 8, true, 14>), dim3(grid), dim3(256), 0, s, devDesc);
        else
          hipLaunchKernelGGL((fusedAggKernel<false, 8, true, 14>), dim3(grid), dim3(256), 0, s, devDesc);
      } else if (desc.wide) {
        hipLaunchKernelGGL((fusedAggKernel<true, 8, false, 14>), dim3(grid), dim3(256), 0, s, devDesc);
      } else {
        hipLaunchKernelGGL((fusedAggKernel<false, 8, false, 14>), dim3(grid), dim3(256), 0, s, devDesc);
      }
    } else if (desc.hasDiv) {
      if (desc.wide) {
        if (small)
          hipLaunchKernelGGL((fusedAggKernel<true, 5, true>), dim3(grid), dim3(256), 0, s, devDesc);
        else
          hipLaunchKernelGGL((fusedAggKernel<true, 8, true>), dim3(grid), dim3(256), 0, s, devDesc);
      } else {
        if (small)
          hipLaunchKernelGGL((fusedAggKernel<false, 5, true>), dim3(grid), dim3(256), 0, s, devDesc);
        else
          hipLaunchKernelGGL((fusedAggKernel<false, 8, true>), dim3(grid), dim3(256), 0, s, devDesc);
      }
    } else if (desc.wide) {
      if (small)
        hipLaunchKernelGGL((fusedAggKernel<true, 5>), dim3(grid), dim3(256), 0, s, devDesc);
      else
        hipLaunchKernelGGL((fusedAggKernel<true, 8>), dim3(grid), dim3(256), 0, s, devDesc);
    } else {
      if (small)
        hipLaunchKernelGGL((fusedAggKernel<false, 5>), dim3(grid), dim3(256), 0, s, devDesc);
      else
        hipLaunchKernelGGL((fusedAggKernel<false, 8>), dim3(grid), dim3(256), 0, s, devDesc);
    }
  }
  return (int)hipGetLastError();
}

int gxLaunchMemset(void* p, int v, size_t n, void* stream) {
  return (int)hipMemsetAsync(p, v, n, (hipStream_t)stream);
}

static int gridFor(int64_t n) {
  int g = (int)((n + 255) / 256);
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return g;
}

int gxJoinAggPhase(int phase, const JoinAggDesc* devDesc, const JoinAggDesc& h,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (phase) {
    case 0:
      hipLaunchKernelGGL(jaCountBuild0Kernel, dim3(gridFor(h.build0.nRows)),
                         dim3(256), 0, s, devDesc);
      break;
    case 1:
      hipLaunchKernelGGL(jaBuild0Kernel, dim3(gridFor(h.build0.nRows)),
                         dim3(256), 0, s, devDesc);
      break;
    case 2:
      hipLaunchKernelGGL(jaCountBuild1Kernel, dim3(gridFor(h.build1.nRows)),
                         dim3(256), 0, s, devDesc);
      break;
    case 3:
      if (h.chained)
        hipLaunchKernelGGL((jaBuild1Kernel<true>),
                           dim3(gridFor(h.build1.nRows)), dim3(256), 0, s,
                           devDesc);
      else
        hipLaunchKernelGGL((jaBuild1Kernel<false>),
                           dim3(gridFor(h.build1.nRows)), dim3(256), 0, s,
                           devDesc);
      break;
    case 4:
      if (h.chained) {
        if (h.wide)
          hipLaunchKernelGGL((jaProbeKernel<true, true>),
                             dim3(gridFor(h.probe.nRows)), dim3(256), 0, s,
                             devDesc);
        else
          hipLaunchKernelGGL((jaProbeKernel<false, true>),
                             dim3(gridFor(h.probe.nRows)), dim3(256), 0, s,
                             devDesc);
      } else if (h.wide)
        hipLaunchKernelGGL((jaProbeKernel<true, false>), dim3(gridFor(h.probe.nRows)),
                           dim3(256), 0, s, devDesc);
      else
        hipLaunchKernelGGL((jaProbeKernel<false, false>), dim3(gridFor(h.probe.nRows)),
                           dim3(256), 0, s, devDesc);
      break;
    case 5: {
      int64_t n = h.nSlots > 0 ? h.nSlots : (1LL << h.slotsLog2);
      // chained mode: a re-run of the build (wide retry, re-open) MUST see
      // empty chains — stale heads would self-link rows into cycles
      if (h.chained && h.b1Heads)
        hipMemsetAsync(h.b1Heads, 0, (1ULL << h.b1HeadsLog2) * 4, s);
      hipLaunchKernelGGL(jaInitSlotsKernel, dim3((n + 255) / 256), dim3(256), 0, s,
                         h.slots, n);
      break;
    }
    default:
      return -1;
  }
  return (int)hipGetLastError();
}

int gxJoinAggMax(const JoinAggDesc* devDesc, const JoinAggDesc& h, uint64_t* devMax,
                 void* stream) {
  hipLaunchKernelGGL(jaMaxKernel, dim3(gridFor(h.nSlots)), dim3(256), 0,
                     (hipStream_t)stream, devDesc, devMax);
  return (int)hipGetLastError();
}

int gxJoinAggMergeDups(const JoinAggDesc* devDesc, const JoinAggDesc& h,
                       void* stream) {
  hipLaunchKernelGGL(jaMergeDupSlotsKernel, dim3(gridFor(h.nSlots)), dim3(256),
                     0, (hipStream_t)stream, devDesc);
  return (int)hipGetLastError();
}

int gxJoinAggMaxHi(const JoinAggDesc* devDesc, const JoinAggDesc& h,
                   uint64_t* devMaxHi, void* stream) {
  hipLaunchKernelGGL(jaMaxHiKernel, dim3(gridFor(h.nSlots)), dim3(256), 0,
                     (hipStream_t)stream, devDesc, devMaxHi);
  return (int)hipGetLastError();
}

int gxJoinAggHist(const JoinAggDesc* devDesc, const JoinAggDesc& h,
                  uint32_t* devHist, int shift, void* stream) {
  hipLaunchKernelGGL(jaHistKernel, dim3(gridFor(h.nSlots)), dim3(256), 0,
                     (hipStream_t)stream, devDesc, devHist, shift);
  return (int)hipGetLastError();
}

int gxJoinAggCompact(const JoinAggDesc* devDesc, const JoinAggDesc& h,
                     TopNOut* out, uint64_t* outCount, uint64_t thresholdBucket,
                     int shift, uint64_t cap, void* stream) {
  hipLaunchKernelGGL(jaCompactKernel, dim3(gridFor(h.nSlots)), dim3(256),
                     0, (hipStream_t)stream, devDesc, out, outCount,
                     thresholdBucket, shift, cap);
  return (int)hipGetLastError();
}

int gxGenOrders(DevTable* tab, int64_t rowBegin, int64_t nRows, uint64_t seed,
                int64_t totalRows, void* stream) {
  hipLaunchKernelGGL(genOrdersKernel, dim3(gridFor(nRows)), dim3(256), 0,
                     (hipStream_t)stream, *tab, rowBegin, nRows, seed, totalRows);
  return (int)hipGetLastError();
}

int gxGenCustomerOffsets(DevTable* tab, int64_t rowBegin, int64_t nRows,
                         uint64_t seed, void* stream, long long* totalBytes) {
  hipStream_t s = (hipStream_t)stream;
  // lens in the offsets buffer's tail is unsafe; use a scratch buffer
  int64_t* lens = nullptr;
  if (hipMalloc(&lens, (nRows + 1) * 8) != hipSuccess) return -2;
  hipLaunchKernelGGL(genCustomerLenKernel, dim3(gridFor(nRows)), dim3(256), 0, s,
                     lens, rowBegin, nRows, seed);
  hipMemsetAsync(lens + nRows, 0, 8, s);
  void* tmp = nullptr;
  size_t tmpBytes = 0;
  hipcub::DeviceScan::ExclusiveSum(nullptr, tmpBytes, lens, tab->cols[1].offsets,
                                   nRows + 1, s);
  if (hipMalloc(&tmp, tmpBytes) != hipSuccess) { hipFree(lens); return -2; }
  hipcub::DeviceScan::ExclusiveSum(tmp, tmpBytes, lens, tab->cols[1].offsets,
                                   nRows + 1, s);
  long long total = 0;
  hipError_t e = hipMemcpyAsync(&total, tab->cols[1].offsets + nRows, 8,
                                hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  hipFree(tmp);
  hipFree(lens);
  if (e != hipSuccess) return (int)e;
  *totalBytes = total;
  return (int)hipGetLastError();
}

int gxGenCustomerFill(DevTable* tab, int64_t rowBegin, int64_t nRows,
                      uint64_t seed, void* stream) {
  hipLaunchKernelGGL(genCustomerFillKernel, dim3(gridFor(nRows)), dim3(256), 0,
                     (hipStream_t)stream, *tab, rowBegin, nRows, seed);
  return (int)hipGetLastError();
}

}  // namespace gxp

namespace gxp {

// ---- device full sort support (sortexec/sort.go analog) ----

__global__ void sortIotaKernel(uint32_t* idx, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    idx[i] = (uint32_t)i;
}

// order-preserving u64 key for one sort column, gathered through idx so each
// stable LSD pass sorts the CURRENT permutation by the next-outer key
__global__ void sortComposeKeysKernel(DevTable tab, SortKeyCompose k,
                                      const uint32_t* __restrict__ idx,
                                      uint64_t* __restrict__ keys, int64_t n,
                                      uint32_t* errFlag) {
  const DevCol& c = tab.cols[k.col];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = idx[i];
    uint64_t key;
    if (colIsNull(c, row)) {
      // the bytes under a NULL are not data (AppendNull leaves the previous
      // value there): every NULL composes the key of a zero value, so the
      // stable value pass keeps NULL rows in inner-key order and no error
      // flag can come from them; the null-bit pass then places them
      key = (k.kind == 1 || k.kind == 2 || k.kind == 4)
                ? 0 : 0x8000000000000000ULL;
    } else if (k.kind == 4) {  // general varlen: its dense rank (gx_strkey.h)
      key = k.rank[row];
    } else if (k.kind == 5) {  // f64: order-preserving IEEE bits
      key = f64OrderKey(gptr<uint64_t>(c.data)[row]);
    } else if (k.kind == 0) {  // int64: flip sign bit
      key = gptr<uint64_t>(c.data)[row] ^ 0x8000000000000000ULL;
    } else if (k.kind == 1) {  // packed CoreTime: masked compare order
      key = gptr<uint64_t>(c.data)[row] & ~0xFULL;
    } else if (k.kind == 2) {  // dense char(1); PAD SPACE: ' ' == ''
      uint8_t b = gptr<uint8_t>(c.data)[row];
      key = b == ' ' ? 0 : b;
    } else {  // decimal -> int64 units at the column's declared frac
      typename VT<false>::T v = 0;
      int sc = 0;
      if (!parseDecimalRaw<false>(
              ulonglong2{gptr<uint64_t>(c.data)[row * 40 / 8],
                         gptr<uint64_t>((const uint8_t*)c.data + row * 40 + 8)[0]},
              &v, &sc, errFlag))
        v = 0;  // flag set; result unusable anyway
      if (sc != c.frac) {
        bool ovf = false;
        if (sc < c.frac) v = VT<false>::scale10(v, c.frac - sc, &ovf);
        if (ovf || sc > c.frac) atomicOr(errFlag, kErrScale);
      }
      key = (uint64_t)v ^ 0x8000000000000000ULL;
    }
    if (k.desc) key = ~key;
    keys[i] = key;
  }
}

// ==================================================================
// standalone hash join (inner, duplicate build keys) — HashJoinDesc
// ==================================================================

// load a row's 1-2 fixed 8-byte key columns; false if any is NULL
// (NULL join keys never match, inner_join_probe.go)
__device__ inline bool hjLoadKeys(const HashJoinDesc& d, const DevTable& t,
                                  const int32_t* cols, int64_t row,
                                  uint64_t* k0, uint64_t* k1) {
  const DevCol& c0 = t.cols[cols[0]];
  if (colIsNull(c0, row)) return false;
  *k0 = gptr<uint64_t>(c0.data)[row];
  *k1 = 0;
  if (d.nKeys > 1) {
    const DevCol& c1 = t.cols[cols[1]];
    if (colIsNull(c1, row)) return false;
    *k1 = gptr<uint64_t>(c1.data)[row];
  }
  return true;
}

__device__ inline uint64_t hjHash(const HashJoinDesc& d, uint64_t k0,
                                  uint64_t k1) {
  uint64_t h = hashKey(k0);
  if (d.nKeys > 1) h = splitmix64(h ^ k1);
  return h;
}

// chain member's keys == probe keys? (rows with NULL keys never entered the
// chain, so no null checks here)
__device__ inline bool hjBuildKeyEq(const HashJoinDesc& d, uint32_t brow,
                                    uint64_t k0, uint64_t k1) {
  if (gptr<uint64_t>(d.build.cols[d.bKeyCol[0]].data)[brow] != k0) return false;
  if (d.nKeys > 1 &&
      gptr<uint64_t>(d.build.cols[d.bKeyCol[1]].data)[brow] != k1)
    return false;
  return true;
}

// ---- general join keys (SerializeKeys semantics, codec.go:852-910) ----
// Per-column canonical values: raw 8 B (kind 0), value-normalized decimal
// (kind 1 — units with trailing zeros stripped + residual scale, ToHashKey
// semantics so 1.10 == 1.1 across fracs), PAD-SPACE-trimmed varlen string
// (kind 2, compared byte-wise against the resident build column).
struct HjKeyVals {
  uint64_t lo[kMaxJoinKeys];   // raw value | decimal units lo | string trimmed len
  int64_t hi[kMaxJoinKeys];    // decimal units hi
  int32_t sc[kMaxJoinKeys];    // decimal residual scale
  int64_t soff[kMaxJoinKeys];  // string byte start in the probe-side data
};

__device__ inline bool hjDecCanon(const DevCol& c, int64_t row, uint64_t* lo,
                                  int64_t* hi, int32_t* sc, uint32_t* err) {
  Int128 u;
  int scale;
  if (!loadDecimalUnits<true>((const uint8_t*)c.data + row * 40, &u, &scale,
                              err))
    return false;
  __int128 v = ((__int128)u.hi << 64) | u.lo;
  bool neg = v < 0;
  unsigned __int128 a = (unsigned __int128)(neg ? -v : v);
  while (scale > 0) {
    unsigned __int128 q = u128DivU64(a, 10);
    if (q * 10 != a) break;
    a = q;
    scale--;
  }
  __int128 r = neg ? -(__int128)a : (__int128)a;
  *lo = (uint64_t)r;
  *hi = (int64_t)(r >> 64);
  *sc = scale;
  return true;
}

__device__ inline bool hjLoadKeysG(const HashJoinDesc& d, const DevTable& t,
                                   const int32_t* cols, int64_t row,
                                   HjKeyVals* v, uint64_t* hash) {
  uint64_t h = 0x243F6A8885A308D3ULL;
  for (int k = 0; k < d.nKeys; k++) {
    const DevCol& c = t.cols[cols[k]];
    if (colIsNull(c, row)) return false;
    int kind = d.keyKind[k];
    if (kind == 0) {
      uint64_t x = gptr<uint64_t>(c.data)[row];
      v->lo[k] = x;
      h = splitmix64(h ^ x);
    } else if (kind == 1) {
      if (!hjDecCanon(c, row, &v->lo[k], &v->hi[k], &v->sc[k], d.errorFlag))
        return false;
      h = splitmix64(h ^ v->lo[k]);
      h = splitmix64(h ^ (uint64_t)v->hi[k]);
      h = splitmix64(h ^ (uint64_t)(uint32_t)v->sc[k]);
    } else {
      int64_t s = gptr<int64_t>(c.offsets)[row];
      int64_t e = gptr<int64_t>(c.offsets)[row + 1];
      auto p = gptr<uint8_t>(c.data);
      while (e > s && p[e - 1] == ' ') e--;
      v->lo[k] = (uint64_t)(e - s);
      v->soff[k] = s;
      for (int64_t j = s; j < e; j += 8) {
        uint64_t w = 0;
        int64_t m = e - j < 8 ? e - j : 8;
        for (int64_t tt = 0; tt < m; tt++)
          w |= (uint64_t)p[j + tt] << (8 * tt);
        h = splitmix64(h ^ w);
      }
      h = splitmix64(h ^ (v->lo[k] * 0x9E3779B97F4A7C15ULL + 1));
    }
  }
  *hash = h;
  return true;
}

__device__ inline bool hjBuildKeyEqG(const HashJoinDesc& d, uint32_t brow,
                                     const HjKeyVals& pv) {
  for (int k = 0; k < d.nKeys; k++) {
    const DevCol& c = d.build.cols[d.bKeyCol[k]];
    int kind = d.keyKind[k];
    if (kind == 0) {
      if (gptr<uint64_t>(c.data)[brow] != pv.lo[k]) return false;
    } else if (kind == 1) {
      uint64_t lo;
      int64_t hi;
      int32_t sc;
      if (!hjDecCanon(c, brow, &lo, &hi, &sc, d.errorFlag)) return false;
      if (lo != pv.lo[k] || hi != pv.hi[k] || sc != pv.sc[k]) return false;
    } else {
      int64_t s = gptr<int64_t>(c.offsets)[brow];
      int64_t e = gptr<int64_t>(c.offsets)[brow + 1];
      auto bp = gptr<uint8_t>(c.data);
      while (e > s && bp[e - 1] == ' ') e--;
      if ((uint64_t)(e - s) != pv.lo[k]) return false;
      auto pp = gptr<uint8_t>(d.probe.cols[d.pKeyCol[k]].data);
      for (int64_t j = 0; j < e - s; j++)
        if (bp[s + j] != pp[pv.soff[k] + j]) return false;
    }
  }
  return true;
}

// key storage + load/eq shims shared by the fast (2 x u64 registers) and
// general (HjKeyVals) kernel variants
template <bool G>
struct HjKeys;
template <>
struct HjKeys<false> {
  uint64_t k0 = 0, k1 = 0;
};
template <>
struct HjKeys<true> {
  HjKeyVals v;
};

__device__ inline bool hjLoad(const HashJoinDesc& d, const DevTable& t,
                              const int32_t* cols, int64_t row,
                              HjKeys<false>& K, uint64_t* h) {
  if (!hjLoadKeys(d, t, cols, row, &K.k0, &K.k1)) return false;
  *h = hjHash(d, K.k0, K.k1);
  return true;
}
__device__ inline bool hjLoad(const HashJoinDesc& d, const DevTable& t,
                              const int32_t* cols, int64_t row,
                              HjKeys<true>& K, uint64_t* h) {
  return hjLoadKeysG(d, t, cols, row, &K.v, h);
}
__device__ inline bool hjEq(const HashJoinDesc& d, uint32_t brow,
                            const HjKeys<false>& K) {
  return hjBuildKeyEq(d, brow, K.k0, K.k1);
}
__device__ inline bool hjEq(const HashJoinDesc& d, uint32_t brow,
                            const HjKeys<true>& K) {
  return hjBuildKeyEqG(d, brow, K.v);
}

// chain-insert every qualifying build row (lock-free head CAS; the next[]
// write is published to the probe kernels by the dispatch boundary)
template <bool G>
__global__ void hjBuildKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.build.nRows;
  uint32_t mask = (1u << d.headsLog2) - 1;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPredB == 0 ||
                evalSimplePred(d.build, d.predB, d.strConstB, d.strConstBLen, row);
    if (!pass) continue;
    HjKeys<G> K;
    uint64_t h;
    if (!hjLoad(d, d.build, d.bKeyCol, row, K, &h)) continue;
    uint32_t slot = (uint32_t)(h & mask);
    uint32_t newHead = (uint32_t)row + 1;
    uint32_t old = d.heads[slot];
    for (;;) {
      d.next[row] = old;
      uint32_t prev = atomicCAS(&d.heads[slot], old, newHead);
      if (prev == old) break;
      old = prev;
    }
  }
}

// probe: walk the chain comparing build keys loaded straight from the
// resident build column. FILL=false counts (wavefront-reduced into
// counters[0]); FILL=true reserves a contiguous range per probe row via one
// atomic on counters[1] and writes the (build,probe) match pairs.
template <bool FILL, bool G = false>
__global__ void hjProbeKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.probe.nRows;
  uint32_t mask = (1u << d.headsLog2) - 1;
  int lane = threadIdx.x & 63;
  uint64_t my = 0;
  // wave-uniform loop: FILL reserves output ranges with ONE atomic per
  // wavefront (a per-row atomic on the shared cursor serializes ~100M
  // atomics/s — measured 369 ms at 30M rows before aggregation)
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;;
       row += stride) {
    bool active = row < n;
    if (__ballot(active) == 0) break;
    if (FILL && d.joinType >= 6) {
      // left outer semi: hits already IS the scalar; one output row per
      // eligible probe row, outBuild carries the flag (0/1/2=NULL)
      uint32_t enc = active ? gptr<uint32_t>(d.hits)[row] : kHjIneligible;
      uint64_t emit = enc != kHjIneligible ? 1 : 0;
      uint64_t pre = emit;
      for (int off = 1; off < 64; off <<= 1) {
        uint64_t t = __shfl_up(pre, off, 64);
        if (lane >= off) pre += t;
      }
      if (emit) {
        uint64_t base =
            (uint64_t)gptr<int64_t>(d.tileBases)[(row - lane) >> 6] +
            (pre - emit);
        d.outBuild[base] = enc;
        d.outProbe[base] = (uint32_t)row;
      }
      continue;
    }
    uint32_t cnt = 0;
    uint32_t head = 0;
    bool pass = false;
    bool needWalk = false;
    HjKeys<G> K;
    // matched rows are cached in registers during the walk so the common
    // case (a handful of duplicates) never re-walks the chain; the FILL
    // pass walks NO chain for rows the count pass resolved to 0/1 matches —
    // it streams the cached per-row hits and the scanned tile bases instead
    // (the r01 fill spent 12.5 ms on wave-serialized cursor atomics + a
    // full re-walk)
    uint32_t hit[4];
    if (active) {
      if (FILL) {
        uint32_t enc = gptr<uint32_t>(d.hits)[row];
        pass = enc != kHjIneligible;
        if (enc != 0 && enc != kHjIneligible) {
          if (enc != kHjMulti) {
            cnt = 1;
            hit[0] = enc - 1;
          } else {
            needWalk = true;
          }
        }
      } else {
        pass = d.nPredP == 0 ||
               evalSimplePred(d.probe, d.predP, d.strConstP, d.strConstPLen,
                              row);
        needWalk = pass;
      }
      if (needWalk) {
        uint64_t h;
        if (!hjLoad(d, d.probe, d.pKeyCol, row, K, &h)) {
          if (d.joinType == 5) pass = false;  // NAAJ: NULL key rejects
        } else {
          head = gptr<uint32_t>(d.heads)[(uint32_t)(h & mask)];
          for (uint32_t cur = head; cur != 0;) {
            uint32_t brow = cur - 1;
            if (hjEq(d, brow, K)) {
              if (cnt < 4) hit[cnt] = brow;
              if (!FILL && d.joinType == 2)  // right outer: flag during count
                atomicOr(&d.matched[brow >> 5], 1u << (brow & 31));
              cnt++;
            }
            cur = gptr<uint32_t>(d.next)[brow];
          }
        }
      }
      if (!FILL)  // cache the walk result for the fill pass
        d.hits[row] = !pass      ? kHjIneligible
                      : cnt == 0 ? 0u
                      : cnt == 1 ? hit[0] + 1
                                 : kHjMulti;
    }
    // per-join-type output rows for this probe row (pred-failing rows emit
    // nothing regardless of type)
    uint32_t emit = active ? cnt : 0;
    bool nullExt = false;
    if (active) {
      if (d.joinType == 1) {  // left outer: unmatched probe null-extends
        if (pass && cnt == 0) { emit = 1; nullExt = true; }
      } else if (d.joinType == 3) {  // semi: once on any match
        emit = cnt ? 1 : 0;
      } else if (d.joinType >= 4) {  // anti semi / null-aware: no match
        emit = (pass && cnt == 0) ? 1 : 0;
        nullExt = emit != 0;
      }
    }
    if (FILL) {
      // deterministic base = scanned tile base + intra-wave exclusive
      // prefix (wave rows are contiguous, so tile = lane-0 row / 64)
      uint64_t pre = emit;
      for (int off = 1; off < 64; off <<= 1) {
        uint64_t t = __shfl_up(pre, off, 64);
        if (lane >= off) pre += t;
      }
      if (emit == 0) continue;
      uint64_t base =
          (uint64_t)gptr<int64_t>(d.tileBases)[(row - lane) >> 6] +
          (pre - emit);
      if (nullExt) {
        d.outBuild[base] = kHjNullRow;
        d.outProbe[base] = (uint32_t)row;
      } else if (d.joinType == 3) {
        d.outBuild[base] = hit[0];
        d.outProbe[base] = (uint32_t)row;
      } else if (cnt <= 4) {
        for (uint32_t k = 0; k < cnt; k++) {
          d.outBuild[base + k] = hit[k];
          d.outProbe[base + k] = (uint32_t)row;
        }
      } else {
        for (uint32_t cur = head; cur != 0;) {
          uint32_t brow = cur - 1;
          if (hjEq(d, brow, K)) {
            d.outBuild[base] = brow;
            d.outProbe[base] = (uint32_t)row;
            base++;
          }
          cur = gptr<uint32_t>(d.next)[brow];
        }
      }
    } else {
      my += emit;
      // per-tile emit total for the fill pass's deterministic bases
      uint64_t tot = emit;
      for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
      if (lane == 0 && row < n) d.tileCounts[row >> 6] = (int64_t)tot;
    }
  }
  if (!FILL) {
    for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
    if (lane == 0 && my)
      atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
  }
}

// evaluate the post-join CNF on one match pair; NULL operands reject
// (VecEvalBool semantics)
__device__ inline bool hjPostOne(const HashJoinDesc& d,
                                 const JoinPostPred& q, uint32_t brow,
                                 uint32_t prow) {
    if (q.kind == 0) {
      const DevTable& t = q.side == 0 ? d.build : d.probe;
      int64_t row = q.side == 0 ? (int64_t)brow : (int64_t)prow;
      if (!evalSimplePred(t, q.pd, q.strC, q.strCLen, row, d.errorFlag))
        return false;
    } else {
      int nbc = d.build.nCols;
      const DevCol& lc = q.lcol < nbc ? d.build.cols[q.lcol]
                                      : d.probe.cols[q.lcol - nbc];
      const DevCol& rc = q.rcol < nbc ? d.build.cols[q.rcol]
                                      : d.probe.cols[q.rcol - nbc];
      int64_t lrow = q.lcol < nbc ? (int64_t)brow : (int64_t)prow;
      int64_t rrow = q.rcol < nbc ? (int64_t)brow : (int64_t)prow;
      if (colIsNull(lc, lrow) || colIsNull(rc, rrow)) return false;
      int c;
      if (q.ctype == 3 /*GX_TYPE_TIME*/) {
        uint64_t a = gptr<uint64_t>(lc.data)[lrow] & ~0xFULL;
        uint64_t b = gptr<uint64_t>(rc.data)[rrow] & ~0xFULL;
        c = a < b ? -1 : (a > b ? 1 : 0);
      } else {
        int64_t a = gptr<int64_t>(lc.data)[lrow];
        int64_t b = gptr<int64_t>(rc.data)[rrow];
        c = a < b ? -1 : (a > b ? 1 : 0);
      }
      if (!cmpResult(c, q.cmp)) return false;
    }
  return true;
}

__device__ inline bool hjPostPass(const HashJoinDesc& d, uint32_t brow,
                                  uint32_t prow) {
  // CNF of disjunction groups: a conjunct passes when ANY of its OR'd
  // entries passes (LogicOr; a NULL leaf counts false on both sides)
  for (int p = 0; p < d.nPost;) {
    int n = d.post[p].orWith + 1;
    bool ok = false;
    for (int j = 0; j < n && !ok; j++)
      ok = hjPostOne(d, d.post[p + j], brow, prow);
    if (!ok) return false;
    p += n;
  }
  return true;
}

// compact filter-surviving match pairs (wave-aggregated cursor, one atomic
// per wavefront)
__global__ void hjFilterPairsKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.nPairs;
  int lane = threadIdx.x & 63;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;;
       i += stride) {
    bool active = i < n;
    if (__ballot(active) == 0) break;
    uint32_t brow = 0, prow = 0;
    bool keep = false;
    if (active) {
      brow = gptr<uint32_t>(d.outBuild)[i];
      prow = gptr<uint32_t>(d.outProbe)[i];
      keep = hjPostPass(d, brow, prow);
    }
    uint64_t m = __ballot(keep);
    if (m == 0) continue;
    uint64_t base = 0;
    if (lane == 0)
      base = atomicAdd((unsigned long long*)&d.counters[2],
                       (unsigned long long)__popcll(m));
    base = __shfl(base, 0, 64);
    if (keep) {
      uint64_t off = __popcll(m & ((1ULL << lane) - 1));
      d.outBuild2[base + off] = brow;
      d.outProbe2[base + off] = prow;
    }
  }
}

// null-aware anti semi (x NOT IN (...)): the probe outcome depends on two
// build-side scalars — how many rows pass the build filter, and how many of
// those have a NULL key (null_aware NAASJ, hash_join_v1.go:599). Count both.
template <bool G>
__global__ void hjBuildStatsKernel(const HashJoinDesc* __restrict__ dp,
                                   uint64_t* __restrict__ out2) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.build.nRows;
  uint64_t myPass = 0, myNull = 0;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool pass = d.nPredB == 0 ||
                evalSimplePred(d.build, d.predB, d.strConstB, d.strConstBLen, row);
    if (!pass) continue;
    myPass++;
    HjKeys<G> K;
    uint64_t h;
    if (!hjLoad(d, d.build, d.bKeyCol, row, K, &h)) myNull++;
  }
  for (int off = 32; off > 0; off >>= 1) {
    myPass += __shfl_down(myPass, off, 64);
    myNull += __shfl_down(myNull, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (myPass) atomicAdd((unsigned long long*)&out2[0],
                          (unsigned long long)myPass);
    if (myNull) atomicAdd((unsigned long long*)&out2[1],
                          (unsigned long long)myNull);
  }
}

// materialize the left-outer-semi scalar column from the flag-encoded
// match array (one byte of null bitmap per 8 output rows; LSB-first 1=valid)
__global__ void hjFlagColKernel(const uint32_t* __restrict__ enc, int64_t n,
                                int64_t* __restrict__ data,
                                uint8_t* __restrict__ nullBitmap) {
  int64_t nBytes = (n + 7) / 8;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nBytes;
       b += (int64_t)gridDim.x * blockDim.x) {
    uint8_t bits = 0;
    for (int j = 0; j < 8; j++) {
      int64_t i = b * 8 + j;
      if (i >= n) break;
      uint32_t e = gptr<uint32_t>(enc)[i];
      data[i] = e == 1 ? 1 : 0;
      if (e != 2) bits |= (uint8_t)(1u << j);
    }
    nullBitmap[b] = bits;
  }
}

int gxHjFlagCol(const uint32_t* enc, int64_t n, int64_t* data,
                uint8_t* nullBitmap, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(hjFlagColKernel, dim3(gridFor((n + 7) / 8)), dim3(256),
                     0, (hipStream_t)stream, enc, n, data, nullBitmap);
  return (int)hipGetLastError();
}

int gxHjBuildStats(const HashJoinDesc* devDesc, const HashJoinDesc& h,
                   uint64_t* out2, void* stream) {
  int64_t n = h.build.nRows;
  if (n == 0) return 0;
  if (h.generalKeys)
    hipLaunchKernelGGL(hjBuildStatsKernel<true>, dim3(gridFor(n)), dim3(256),
                       0, (hipStream_t)stream, devDesc, out2);
  else
    hipLaunchKernelGGL(hjBuildStatsKernel<false>, dim3(gridFor(n)), dim3(256),
                       0, (hipStream_t)stream, devDesc, out2);
  return (int)hipGetLastError();
}

// out-of-core join (hash_join_spill.go analog): per-row partition id from
// the join-key hash, using bits independent of the chain-table index so the
// per-partition tables hash freely. NULL-key rows round-robin by row index —
// they match nothing, but outer/anti joins still emit them.
template <bool G>
__global__ void hjPartIdKernel(const HashJoinDesc* __restrict__ dp, int side,
                               int nParts, uint32_t* __restrict__ out) {
  const HashJoinDesc& d = *dp;
  const DevTable& t = side == 0 ? d.build : d.probe;
  const int32_t* cols = side == 0 ? d.bKeyCol : d.pKeyCol;
  int64_t n = t.nRows;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    HjKeys<G> K;
    uint64_t h;
    uint32_t p;
    if (hjLoad(d, t, cols, row, K, &h))
      p = (uint32_t)((h >> 43) % (uint64_t)nParts);
    else
      p = (uint32_t)(row % nParts);
    out[row] = p;
  }
}

int gxHjPartIds(const HashJoinDesc* devDesc, const HashJoinDesc& h, int side,
                int nParts, uint32_t* out, void* stream) {
  int64_t n = side == 0 ? h.build.nRows : h.probe.nRows;
  if (n == 0) return 0;
  if (h.generalKeys)
    hipLaunchKernelGGL(hjPartIdKernel<true>, dim3(gridFor(n)), dim3(256), 0,
                       (hipStream_t)stream, devDesc, side, nParts, out);
  else
    hipLaunchKernelGGL(hjPartIdKernel<false>, dim3(gridFor(n)), dim3(256), 0,
                       (hipStream_t)stream, devDesc, side, nParts, out);
  return (int)hipGetLastError();
}

// ---- paired count pass ----
// Each chain step is a dependent random cache line, so the count pass is
// latency-bound; walking TWO rows' chains in lock-step per thread doubles
// the loads in flight (count measured 4.3 ms at SF10 against a ~1.8 ms
// random-line floor).
template <bool G>
__device__ inline void hjCountProlog(const HashJoinDesc& d, int64_t row,
                                     uint32_t mask, bool* pass,
                                     uint32_t* cur, HjKeys<G>* K,
                                     bool* keyNull) {
  *pass = d.nPredP == 0 || evalSimplePred(d.probe, d.predP, d.strConstP,
                                          d.strConstPLen, row);
  *cur = 0;
  *keyNull = false;
  uint64_t h;
  if (*pass && hjLoad(d, d.probe, d.pKeyCol, row, *K, &h)) {
    *cur = gptr<uint32_t>(d.heads)[(uint32_t)(h & mask)];
  } else if (*pass) {
    *keyNull = true;
    if (d.joinType == 5)
      *pass = false;  // null-aware anti semi: NULL probe key -> NOT IN is
                      // NULL -> reject (null_aware NAASJ, hash_join_v1.go)
  }
}

__device__ inline uint32_t hjCountEmit(const HashJoinDesc& d, bool active,
                                       bool pass, uint32_t cnt) {
  if (!active) return 0;
  if (d.joinType == 1) return pass && cnt == 0 ? 1 : cnt;  // left outer
  if (d.joinType == 3) return cnt ? 1 : 0;                 // semi
  if (d.joinType == 4 || d.joinType == 5)
    return pass && cnt == 0 ? 1 : 0;  // anti semi / null-aware anti semi
  if (d.joinType >= 6) return pass ? 1 : 0;  // left outer semi: the scalar
  return cnt;
}

template <bool G>
__global__ void hjCountKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.probe.nRows;
  uint32_t mask = (1u << d.headsLog2) - 1;
  int lane = threadIdx.x & 63;
  uint64_t my = 0;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t rowA = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;;
       rowA += 2 * stride) {
    int64_t rowB = rowA + stride;
    bool actA = rowA < n, actB = rowB < n;
    if (__ballot(actA) == 0) break;  // actB implies actA
    bool passA = false, passB = false;
    uint32_t curA = 0, curB = 0;
    HjKeys<G> KA, KB;
    bool knA = false, knB = false;
    if (actA) hjCountProlog(d, rowA, mask, &passA, &curA, &KA, &knA);
    if (actB) hjCountProlog(d, rowB, mask, &passB, &curB, &KB, &knB);
    uint32_t cntA = 0, cntB = 0, hit0A = 0, hit0B = 0;
    while (curA != 0 || curB != 0) {
      if (curA != 0) {
        uint32_t br = curA - 1;
        if (hjEq(d, br, KA)) {
          if (cntA == 0) hit0A = br;
          if (d.joinType == 2)
            atomicOr(&d.matched[br >> 5], 1u << (br & 31));
          cntA++;
        }
        curA = gptr<uint32_t>(d.next)[br];
      }
      if (curB != 0) {
        uint32_t br = curB - 1;
        if (hjEq(d, br, KB)) {
          if (cntB == 0) hit0B = br;
          if (d.joinType == 2)
            atomicOr(&d.matched[br >> 5], 1u << (br & 31));
          cntB++;
        }
        curB = gptr<uint32_t>(d.next)[br];
      }
    }
    if (d.joinType >= 6) {
      // left outer semi: hits IS the output scalar (0 / 1 / 2 = NULL);
      // the fill pass streams it straight into the flag column
      auto flag = [&](bool pass, uint32_t cnt, bool kn) -> uint32_t {
        if (!pass) return kHjIneligible;
        if (cnt) return 1u;
        if ((kn && d.naNullIfKeyNull) || d.naNullAlways) return 2u;
        return 0u;
      };
      if (actA) d.hits[rowA] = flag(passA, cntA, knA);
      if (actB) d.hits[rowB] = flag(passB, cntB, knB);
    } else {
      if (actA)
        d.hits[rowA] = !passA      ? kHjIneligible
                       : cntA == 0 ? 0u
                       : cntA == 1 ? hit0A + 1
                                   : kHjMulti;
      if (actB)
        d.hits[rowB] = !passB      ? kHjIneligible
                       : cntB == 0 ? 0u
                       : cntB == 1 ? hit0B + 1
                                   : kHjMulti;
    }
    uint32_t emitA = hjCountEmit(d, actA, passA, cntA);
    uint32_t emitB = hjCountEmit(d, actB, passB, cntB);
    my += emitA + emitB;
    uint64_t totA = emitA, totB = emitB;
    for (int off = 32; off > 0; off >>= 1) {
      totA += __shfl_down(totA, off, 64);
      totB += __shfl_down(totB, off, 64);
    }
    if (lane == 0 && rowA < n) d.tileCounts[rowA >> 6] = (int64_t)totA;
    if (lane == 0 && rowB < n) d.tileCounts[rowB >> 6] = (int64_t)totB;
  }
  for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
  if (lane == 0 && my)
    atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
}

// right outer: emit every predB-passing build row whose matched flag is
// unset (NULL-key build rows never entered a chain, so they drain here too).
// FILL=false adds the count into counters[0]; FILL=true reserves slices of
// the shared fill cursor counters[1] and writes (brow, kHjNullRow) pairs.
template <bool FILL>
__global__ void hjUnmatchedKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.build.nRows;
  int lane = threadIdx.x & 63;
  uint64_t my = 0;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;;
       row += stride) {
    bool active = row < n;
    if (__ballot(active) == 0) break;
    bool um = false;
    if (active) {
      bool pass = d.nPredB == 0 || evalSimplePred(d.build, d.predB,
                                                  d.strConstB, d.strConstBLen,
                                                  row);
      um = pass &&
           !((gptr<uint32_t>(d.matched)[row >> 5] >> (row & 31)) & 1);
    }
    if (FILL) {
      uint64_t m = __ballot(um);
      if (m == 0) continue;
      uint64_t base = 0;
      if (lane == 63)
        base = atomicAdd((unsigned long long*)&d.counters[1],
                         (unsigned long long)__popcll(m));
      base = __shfl(base, 63, 64) + __popcll(m & ((1ULL << lane) - 1));
      if (um) {
        d.outBuild[base] = (uint32_t)row;
        d.outProbe[base] = kHjNullRow;
      }
    } else {
      my += um ? 1 : 0;
    }
  }
  if (!FILL) {
    for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
    if (lane == 0 && my)
      atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
  }
}

// ---- row-pack gather (gx_common.h RowPackDesc) ----
__global__ void hjPackRowsKernel(RowPackDesc d) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < d.nRows; row += (int64_t)gridDim.x * blockDim.x) {
    uint8_t* out = d.staging + row * (int64_t)d.stride;
    for (int c = 0; c < d.nCols; c++) {
      if (d.width[c] == 8) {
        *(uint64_t*)(out + d.off[c]) = gptr<uint64_t>(d.src[c])[row];
      } else if (d.width[c] == 1) {
        out[d.off[c]] = gptr<uint8_t>(d.src[c])[row];
      } else {  // 40
        auto s = gptr<uint64_t>((const uint8_t*)d.src[c] + row * 40);
        uint64_t* o = (uint64_t*)(out + d.off[c]);
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; o[4] = s[4];
      }
    }
  }
}

__global__ void hjUnpackRowsKernel(RowPackDesc d) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < d.total; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t src = gptr<uint32_t>(d.idx)[i];
    if (src == kHjNullRow) {  // null-extended outer-join row -> zeros
      for (int c = 0; c < d.nCols; c++) {
        if (d.width[c] == 8) ((uint64_t*)d.dst[c])[i] = 0;
        else if (d.width[c] == 1) ((uint8_t*)d.dst[c])[i] = 0;
        else {
          uint64_t* o = (uint64_t*)((uint8_t*)d.dst[c] + i * 40);
          o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; o[4] = 0;
        }
      }
      continue;
    }
    auto in = gptr<uint8_t>(d.staging + (int64_t)src * d.stride);
    for (int c = 0; c < d.nCols; c++) {
      if (d.width[c] == 8) {
        ((uint64_t*)d.dst[c])[i] = *(const __attribute__((address_space(1)))
                                         uint64_t*)(in + d.off[c]);
      } else if (d.width[c] == 1) {
        ((uint8_t*)d.dst[c])[i] = in[d.off[c]];
      } else {
        auto s = (const __attribute__((address_space(1))) uint64_t*)(in +
                                                                     d.off[c]);
        uint64_t* o = (uint64_t*)((uint8_t*)d.dst[c] + i * 40);
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; o[4] = s[4];
      }
    }
  }
}

int gxPackRows(const RowPackDesc& d, void* stream) {
  if (d.nRows == 0) return 0;
  hipLaunchKernelGGL(hjPackRowsKernel, dim3(gridFor(d.nRows)), dim3(256), 0,
                     (hipStream_t)stream, d);
  return (int)hipGetLastError();
}

int gxUnpackRows(const RowPackDesc& d, void* stream) {
  if (d.total == 0) return 0;
  hipLaunchKernelGGL(hjUnpackRowsKernel, dim3(gridFor(d.total)), dim3(256), 0,
                     (hipStream_t)stream, d);
  return (int)hipGetLastError();
}

// standalone Selection (SelectionExec, select.go:750-785): compact the rows
// surviving a CNF into a survivor index, MI355X-shaped — no row-at-a-time
// AppendRow copy; output columns gather through the index afterwards.
// Conjuncts ride HashJoinDesc.post evaluated against d.probe (build side
// empty). FILL=false counts into counters[0]; FILL=true reserves
// wave-aggregated slices of counters[1] and writes row indices.
template <bool FILL>
__global__ void selCompactKernel(const HashJoinDesc* __restrict__ dp) {
  const HashJoinDesc& d = *dp;
  int64_t n = d.probe.nRows;
  int lane = threadIdx.x & 63;
  uint64_t my = 0;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;;
       row += stride) {
    bool active = row < n;
    if (__ballot(active) == 0) break;
    bool keep = active && hjPostPass(d, 0, (uint32_t)row);
    if (FILL) {
      uint64_t m = __ballot(keep);
      if (m == 0) continue;
      uint64_t base = 0;
      if (lane == 0)
        base = atomicAdd((unsigned long long*)&d.counters[1],
                         (unsigned long long)__popcll(m));
      base = __shfl(base, 0, 64) + __popcll(m & ((1ULL << lane) - 1));
      if (keep) d.outProbe[base] = (uint32_t)row;
    } else if (keep) {
      my++;
    }
  }
  if (!FILL) {
    for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
    if (lane == 0 && my)
      atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
  }
}

// ==================================================================
// standalone Projection — ProjDesc (gx_common.h)
// ==================================================================

// encode int128 units at `scale` into the canonical 40-byte MyDecimal
// (mirrors the host decFromUnits digit-exactly: integer words
// most-significant-first, frac words left-aligned 9-digit, mydecimal.go
// word layout)
__device__ inline void devDecEncode(__int128 u, int scale,
                                    uint8_t* __restrict__ out40) {
  bool neg = u < 0;
  unsigned __int128 a = neg ? (unsigned __int128)(-u) : (unsigned __int128)u;
  unsigned __int128 pscale = 1;
  for (int s = scale; s > 0; s -= 9)
    pscale *= (uint64_t)kP10(s > 9 ? 9 : s);
  unsigned __int128 ip, fr128;
  if ((pscale >> 64) != 0) {
    ip = u128DivBig(a, pscale);
  } else if (pscale > 1) {
    ip = u128DivU64(a, (uint64_t)pscale);
  } else {
    ip = a;
  }
  fr128 = a - ip * pscale;
  int32_t words[6] = {0};
  int nw = 0;
  if (ip == 0) {
    words[0] = 0;
    nw = 1;
  } else {
    int32_t tmp[6];
    int k = 0;
    while (ip > 0) {
      unsigned __int128 q = u128DivU64(ip, 1000000000u);
      tmp[k++] = (int32_t)(uint64_t)(ip - q * 1000000000u);
      ip = q;
    }
    nw = k;
    for (int i = 0; i < k; i++) words[i] = tmp[k - 1 - i];
  }
  int digitsInt = (nw - 1) * 9;
  {
    int32_t head = words[0];
    int hd = 1;
    while (head >= 10) {
      head /= 10;
      hd++;
    }
    digitsInt += hd;
  }
  out40[0] = (uint8_t)(int8_t)digitsInt;
  out40[1] = (uint8_t)(int8_t)scale;
  out40[2] = (uint8_t)(int8_t)scale;  // resultFrac
  out40[3] = (uint8_t)(neg && a != 0 ? 1 : 0);
  int32_t* wb = (int32_t*)(out40 + 4);
  for (int i = 0; i < 9; i++) wb[i] = 0;
  for (int i = 0; i < nw; i++) wb[i] = words[i];
  if (scale > 0) {
    int fw = (scale + 8) / 9;
    int pad = fw * 9 - scale;
    unsigned __int128 fadj = fr128 * (uint64_t)kP10(pad);
    for (int i = fw - 1; i >= 0; i--) {
      unsigned __int128 q = u128DivU64(fadj, 1000000000u);
      wb[nw + i] = (int32_t)(uint64_t)(fadj - q * 1000000000u);
      fadj = q;
    }
  }
}

// per-row direct-load VM + output materialization
template <bool WIDE>
__global__ void projectKernel(const ProjDesc* __restrict__ dp) {
  const ProjDesc& d = *dp;
  int64_t n = d.table.nRows;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    VmState14<WIDE> vm;
    vm.nullBits = 0;
    bool bad = false;
    bool ovf = false;
    for (int i = 0; i < d.nIns && !bad; i++) {
      const VmIns& ins = d.ins[i];
      switch (ins.op) {
        case VM_LOAD_DEC: {
          const DevCol& c = d.table.cols[ins.a];
          bool nul = colIsNull(c, row);
          typename VT<WIDE>::T v = VT<WIDE>::zero();
          if (!nul) {
            int sc;
            if (!loadDecimalUnits<WIDE>((const uint8_t*)c.data + row * 40, &v,
                                        &sc, d.errorFlag)) {
              bad = true;
              break;
            }
            if (sc != ins.b) {
              if (sc < ins.b) v = VT<WIDE>::scale10(v, ins.b - sc, &ovf);
              else { atomicOr(d.errorFlag, kErrScale); bad = true; break; }
            }
          }
          vm.set(ins.dst, v);
          vm.setNull(ins.dst, nul);
          break;
        }
        case VM_LOAD_I64: {
          const DevCol& c = d.table.cols[ins.a];
          bool nul = colIsNull(c, row);
          vm.set(ins.dst,
                 nul ? VT<WIDE>::zero()
                     : VT<WIDE>::fromI64(gptr<int64_t>(c.data)[row], &ovf));
          vm.setNull(ins.dst, nul);
          break;
        }
        case VM_STRLEN: {
          // LENGTH (builtinLengthSig): byte length, direct offsets read
          const DevCol& c = d.table.cols[ins.a];
          bool nul = colIsNull(c, row);
          int64_t len = 0;
          if (!nul)
            len = c.denseOffsets ? 1
                                 : gptr<int64_t>(c.offsets)[row + 1] -
                                       gptr<int64_t>(c.offsets)[row];
          vm.set(ins.dst,
                 nul ? VT<WIDE>::zero() : VT<WIDE>::fromI64(len, &ovf));
          vm.setNull(ins.dst, nul);
          break;
        }
        case VM_LIKE: {
          // LIKE / NOT LIKE in value context: i64 0/1, NULL string -> NULL
          const DevCol& c = d.table.cols[ins.a];
          bool nul = colIsNull(c, row);
          int64_t r = 0;
          if (!nul)
            r = likeColMatch(c, d.likePats[ins.b], row) != (ins.c != 0) ? 1 : 0;
          vm.set(ins.dst, VT<WIDE>::fromI64(r, &ovf));
          vm.setNull(ins.dst, nul);
          break;
        }
        default:
          if (!vmStep<WIDE, kVmOpsFull>(vm, ins, d.insP10[i], d.constLo,
                                        d.constHi, d.errorFlag, &ovf))
            bad = true;
          break;
      }
    }
    if (ovf) {
      atomicOr(d.errorFlag, WIDE ? kErrOverflow : kErrRetryWide);
      bad = true;
    }
    if (bad) continue;  // flag set; results of this row are discarded anyway
    for (int o = 0; o < d.nOut; o++) {
      bool nul = vm.isNull(d.outReg[o]);
      d.outNotNull[o][row] = nul ? 0 : 1;
      if (d.outType[o] == 2 /*GX_TYPE_DECIMAL*/) {
        uint8_t* out = (uint8_t*)d.outData[o] + row * 40;
        if (nul) {
          for (int i = 0; i < 10; i++) ((uint32_t*)out)[i] = 0;
        } else {
          Int128 ai = VT<WIDE>::toAcc(vm.get(d.outReg[o]));
          devDecEncode(((__int128)ai.hi << 64) | (__int128)ai.lo,
                       d.outScale[o], out);
        }
      } else {
        Int128 ai = VT<WIDE>::toAcc(vm.get(d.outReg[o]));
        ((int64_t*)d.outData[o])[row] = nul ? 0 : (int64_t)ai.lo;
      }
    }
  }
}

__global__ void packNullsKernel(const uint8_t* __restrict__ notNull,
                                uint8_t* __restrict__ bitmap, int64_t n) {
  int64_t nBytes = (n + 7) / 8;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nBytes;
       b += (int64_t)gridDim.x * blockDim.x) {
    int64_t base = b * 8;
    int m = n - base < 8 ? (int)(n - base) : 8;
    uint8_t v = 0;
    for (int j = 0; j < m; j++)
      if (notNull[base + j]) v |= (uint8_t)(1 << j);
    bitmap[b] = v;
  }
}

// gather a null bitmap through the match index: one thread composes one
// output byte (8 rows) — no atomics (LSB-first, 1 = NOT NULL)
__global__ void hjGatherNullsKernel(const uint8_t* __restrict__ in,
                                    const uint32_t* __restrict__ idx,
                                    uint8_t* __restrict__ out, int64_t n) {
  int64_t nBytes = (n + 7) / 8;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nBytes;
       b += (int64_t)gridDim.x * blockDim.x) {
    int64_t base = b * 8;
    int m = n - base < 8 ? (int)(n - base) : 8;
    uint8_t v = 0;
    for (int j = 0; j < m; j++) {
      uint32_t src = idx[base + j];
      if (src == kHjNullRow) continue;  // null-extended row -> NULL
      if (in == nullptr || ((in[src >> 3] >> (src & 7)) & 1))
        v |= (uint8_t)(1 << j);
    }
    out[b] = v;
  }
}

__global__ void iotaI64Kernel(int64_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = i;
}

// varlen gather pass 1: per-output-row byte lengths
__global__ void hjVarlenLensKernel(const int64_t* __restrict__ inOffsets,
                                   const uint32_t* __restrict__ idx,
                                   int64_t* __restrict__ lens, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t src = idx[i];
    lens[i] = src == kHjNullRow ? 0 : inOffsets[src + 1] - inOffsets[src];
  }
}

// varlen gather pass 2: copy bytes (one thread per output row; rows are
// short strings, so per-thread byte loops stay coalesced enough across the
// wave)
__global__ void hjVarlenBytesKernel(const uint8_t* __restrict__ inData,
                                    const int64_t* __restrict__ inOffsets,
                                    const uint32_t* __restrict__ idx,
                                    const int64_t* __restrict__ outOffsets,
                                    uint8_t* __restrict__ outData, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t src = idx[i];
    if (src == kHjNullRow) continue;
    int64_t s = inOffsets[src];
    int64_t len = inOffsets[src + 1] - s;
    int64_t o = outOffsets[i];
    for (int64_t j = 0; j < len; j++) outData[o + j] = inData[s + j];
  }
}

__global__ void sortGatherKernel(const uint8_t* __restrict__ in,
                                 uint8_t* __restrict__ out,
                                 const uint32_t* __restrict__ idx, int64_t n,
                                 int elemSize) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (idx[i] == kHjNullRow) {  // null-extended outer-join row
      if (elemSize == 8) ((uint64_t*)out)[i] = 0;
      else if (elemSize == 1) out[i] = 0;
      else {
        uint64_t* d = (uint64_t*)(out + i * 40);
        d[0] = 0; d[1] = 0; d[2] = 0; d[3] = 0; d[4] = 0;
      }
      continue;
    }
    int64_t src = idx[i];
    if (elemSize == 8) {
      ((uint64_t*)out)[i] = ((const uint64_t*)in)[src];
    } else if (elemSize == 1) {
      out[i] = in[src];
    } else {  // 40B decimal: five 8B words
      const uint64_t* s = (const uint64_t*)(in + src * 40);
      uint64_t* d = (uint64_t*)(out + i * 40);
      d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3]; d[4] = s[4];
    }
  }
}



// null-bit key pass (sortexec compare: NULL < any value — NULLs first on
// ASC, last on DESC; the 1-bit stable pass runs AFTER the column's value
// pass, i.e. more significant)
__global__ void sortComposeNullKeysKernel(const uint8_t* __restrict__ bitmap,
                                          const uint32_t* __restrict__ idx,
                                          uint64_t* __restrict__ keys,
                                          int64_t n, int desc) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t row = idx[i];
    bool isNull = ((bitmap[row >> 3] >> (row & 7)) & 1) == 0;
    keys[i] = desc ? (isNull ? 1 : 0) : (isNull ? 0 : 1);
  }
}

int gxSortComposeNullKeys(const uint8_t* bitmap, const uint32_t* idx,
                          uint64_t* keys, int64_t n, int desc, void* stream) {
  hipLaunchKernelGGL(sortComposeNullKeysKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, bitmap, idx, keys, n, desc);
  return (int)hipGetLastError();
}

int gxSortIota(uint32_t* idx, int64_t n, void* stream) {
  hipLaunchKernelGGL(sortIotaKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, idx, n);
  return (int)hipGetLastError();
}

int gxSortComposeKeys(const DevTable* tab, const DevTable& htab,
                      SortKeyCompose k, const uint32_t* idx, uint64_t* keys,
                      int64_t n, uint32_t* errFlag, void* stream) {
  (void)tab;
  hipLaunchKernelGGL(sortComposeKeysKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, htab, k, idx, keys, n, errFlag);
  return (int)hipGetLastError();
}

// OR / AND reductions over the composed keys: radix passes can skip bit
// positions that are identical across every key (begin_bit = first
// differing bit, end_bit = last + 1) -- dates pack into bits 41..54 and
// dense int keys into the low bits, cutting 8 passes to 2-3.
__global__ void sortKeyBitsKernel(const uint64_t* __restrict__ keys, int64_t n,
                                  uint64_t* orOut, uint64_t* andOut) {
  uint64_t o = 0, a = ~0ULL;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    o |= keys[i];
    a &= keys[i];
  }
  for (int off = 32; off > 0; off >>= 1) {
    o |= __shfl_down(o, off, 64);
    a &= __shfl_down(a, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicOr((unsigned long long*)orOut, (unsigned long long)o);
    atomicAnd((unsigned long long*)andOut, (unsigned long long)a);
  }
}

int gxSortKeyBits(const uint64_t* keys, int64_t n, uint64_t* devOrAnd,
                  void* stream) {
  hipMemsetAsync(devOrAnd, 0, 8, (hipStream_t)stream);
  hipMemsetAsync(devOrAnd + 1, 0xFF, 8, (hipStream_t)stream);
  hipLaunchKernelGGL(sortKeyBitsKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, keys, n, devOrAnd, devOrAnd + 1);
  return (int)hipGetLastError();
}

int gxSortPairs(uint64_t* keysIn, uint64_t* keysOut, uint32_t* idxIn,
                uint32_t* idxOut, int64_t n, void* tmp, size_t* tmpBytes,
                int beginBit, int endBit, void* stream) {
  return (int)hipcub::DeviceRadixSort::SortPairs(tmp, *tmpBytes, keysIn,
                                                 keysOut, idxIn, idxOut,
                                                 (int)n, beginBit, endBit,
                                                 (hipStream_t)stream);
}

int gxSortGatherCol(const void* in, void* out, const uint32_t* idx, int64_t n,
                    int elemSize, void* stream) {
  hipLaunchKernelGGL(sortGatherKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, (const uint8_t*)in, (uint8_t*)out,
                     idx, n, elemSize);
  return (int)hipGetLastError();
}

int gxHashJoinPhase(int phase, const HashJoinDesc* devDesc,
                    const HashJoinDesc& h, void* stream) {
  int64_t rows = (phase == 0 || phase >= 4) ? h.build.nRows
                 : phase == 3               ? h.nPairs
                                            : h.probe.nRows;
  if (rows == 0) return 0;
  dim3 g(gridFor(rows));
  if (phase >= 4) {  // right-outer unmatched-build drain
    if (phase == 4)
      hipLaunchKernelGGL(hjUnmatchedKernel<false>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
    else
      hipLaunchKernelGGL(hjUnmatchedKernel<true>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
    return (int)hipGetLastError();
  }
  const bool gen = h.generalKeys != 0;
  if (phase == 0) {
    if (gen)
      hipLaunchKernelGGL(hjBuildKernel<true>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
    else
      hipLaunchKernelGGL(hjBuildKernel<false>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
  } else if (phase == 1) {
    if (gen)
      hipLaunchKernelGGL(hjCountKernel<true>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
    else
      hipLaunchKernelGGL(hjCountKernel<false>, g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
  } else if (phase == 2) {
    if (gen)
      hipLaunchKernelGGL((hjProbeKernel<true, true>), g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
    else
      hipLaunchKernelGGL((hjProbeKernel<true, false>), g, dim3(256), 0,
                         (hipStream_t)stream, devDesc);
  } else {
    hipLaunchKernelGGL(hjFilterPairsKernel, g, dim3(256), 0,
                       (hipStream_t)stream, devDesc);
  }
  return (int)hipGetLastError();
}

int gxSelectPhase(int phase, const HashJoinDesc* devDesc,
                  const HashJoinDesc& h, void* stream) {
  if (h.probe.nRows == 0) return 0;
  dim3 g(gridFor(h.probe.nRows));
  if (phase == 0)
    hipLaunchKernelGGL(selCompactKernel<false>, g, dim3(256), 0,
                       (hipStream_t)stream, devDesc);
  else
    hipLaunchKernelGGL(selCompactKernel<true>, g, dim3(256), 0,
                       (hipStream_t)stream, devDesc);
  return (int)hipGetLastError();
}

__global__ void strWindowKernel(const ProjDesc* __restrict__ dp, int pi) {
  const ProjDesc& d = *dp;
  const StrProg& sp = d.sprog[pi];
  const DevCol& c = d.table.cols[sp.col];
  int64_t n = d.table.nRows;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    bool nul = colIsNull(c, row);
    int64_t s = 0, len = 0;
    if (!nul) {
      if (c.denseOffsets) {
        s = row;
        len = 1;
      } else {
        s = gptr<int64_t>(c.offsets)[row];
        len = gptr<int64_t>(c.offsets)[row + 1] - s;
      }
      // SUBSTR windows compose, TRIM stays a window (gx_strcat.h)
      auto p = gptr<uint8_t>(c.data);
      strWindowFold(sp.nWin, sp.winPos, sp.winLen, &s, &len,
                    [&](int64_t i) { return p[i]; });
    }
    sp.starts[row] = s;
    sp.lens[row] = len;
    sp.notNull[row] = nul ? 0 : 1;
  }
}

__global__ void strEmitKernel(const ProjDesc* __restrict__ dp, int pi,
                              const int64_t* __restrict__ outOffsets,
                              uint8_t* __restrict__ outData) {
  const ProjDesc& d = *dp;
  const StrProg& sp = d.sprog[pi];
  const DevCol& c = d.table.cols[sp.col];
  int64_t n = d.table.nRows;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = gptr<int64_t>(sp.starts)[row];
    int64_t len = gptr<int64_t>(sp.lens)[row];
    int64_t o = outOffsets[row];
    auto p = gptr<uint8_t>(c.data);
    for (int64_t j = 0; j < len; j++) {
      uint8_t b = p[s + j];
      if (sp.upper && b >= 'a' && b <= 'z') b = (uint8_t)(b - 'a' + 'A');
      if (sp.lower && b >= 'A' && b <= 'Z') b = (uint8_t)(b - 'A' + 'a');
      outData[o + j] = b;
    }
  }
}

int gxStrWindow(const ProjDesc* devDesc, const ProjDesc& h, int progIdx,
                void* stream) {
  if (h.table.nRows == 0) return 0;
  hipLaunchKernelGGL(strWindowKernel, dim3(gridFor(h.table.nRows)), dim3(256),
                     0, (hipStream_t)stream, devDesc, progIdx);
  return (int)hipGetLastError();
}

int gxStrEmit(const ProjDesc* devDesc, const ProjDesc& h, int progIdx,
              const int64_t* outOffsets, uint8_t* outData, void* stream) {
  if (h.table.nRows == 0) return 0;
  hipLaunchKernelGGL(strEmitKernel, dim3(gridFor(h.table.nRows)), dim3(256),
                     0, (hipStream_t)stream, devDesc, progIdx, outOffsets,
                     outData);
  return (int)hipGetLastError();
}

// ---- composed string outputs (CONCAT / CONCAT_WS / CAST_STR) ----
// Both kernels run the piece table and byte mapping of gx_strcat.h. The
// program, the constant pool and the WINDOW pieces' column data pointers are
// staged in LDS once per block (as raw bytes: StrCatProg has member
// initializers, which a __shared__ object may not run).
struct CatStage {
  StrCatProg prog;
  uint8_t pool[kStrCatPoolBytes];
  const uint8_t* data[kStrCatMaxPieces];
};

__device__ inline void catStageLoad(CatStage& st, const ProjDesc& d, int ci) {
  static_assert(sizeof(StrCatProg) % 4 == 0, "copied by words");
  const uint32_t* src = (const uint32_t*)&d.cat[ci];
  uint32_t* dst = (uint32_t*)&st.prog;
  for (int i = threadIdx.x; i < (int)(sizeof(StrCatProg) / 4); i += blockDim.x)
    dst[i] = src[i];
  for (int i = threadIdx.x; i < kStrCatPoolBytes; i += blockDim.x)
    st.pool[i] = d.catPool[i];
  if (threadIdx.x < kStrCatMaxPieces) {
    const StrPiece& pc = d.cat[ci].piece[threadIdx.x];
    bool win = (int)threadIdx.x < d.cat[ci].nPieces && pc.kind == SPK_WINDOW;
    st.data[threadIdx.x] =
        win ? (const uint8_t*)d.table.cols[pc.col].data : nullptr;
  }
  __syncthreads();
}

struct CatDevSrc {
  const ProjDesc& d;
  const CatStage& st;
  __device__ bool strNull(int p, int64_t row) const {
    return colIsNull(d.table.cols[st.prog.piece[p].col], row);
  }
  __device__ void strRange(int p, int64_t row, int64_t* s, int64_t* len) const {
    const DevCol& c = d.table.cols[st.prog.piece[p].col];
    if (c.denseOffsets) {
      *s = row;
      *len = 1;
    } else {
      *s = gptr<int64_t>(c.offsets)[row];
      *len = gptr<int64_t>(c.offsets)[row + 1] - *s;
    }
  }
  __device__ uint8_t strByte(int p, int64_t i) const {
    return gptr<uint8_t>(st.data[p])[i];
  }
  __device__ bool i64At(int p, int64_t row, int64_t* v) const {
    const StrPiece& pc = st.prog.piece[p];
    if (pc.col >= 0) {  // a plain int64 column reads the table directly
      const DevCol& c = d.table.cols[pc.col];
      if (colIsNull(c, row)) return false;
      *v = gptr<int64_t>(c.data)[row];
      return true;
    }
    if (gptr<uint8_t>(d.outNotNull[pc.slot])[row] == 0) return false;
    *v = gptr<int64_t>(d.outData[pc.slot])[row];
    return true;
  }
  __device__ uint8_t pool(int i) const { return st.pool[i]; }
};

// length pass: one lane per row, 9 B/row out, no per-piece temporaries
__global__ __launch_bounds__(256) void strCatLensKernel(
    const ProjDesc* __restrict__ dp, int ci, int64_t* __restrict__ lens,
    uint8_t* __restrict__ notNull) {
  __shared__ __align__(16) uint8_t stRaw[sizeof(CatStage)];
  CatStage& st = *reinterpret_cast<CatStage*>(stRaw);
  const ProjDesc& d = *dp;
  catStageLoad(st, d, ci);
  CatDevSrc src{d, st};
  int64_t n = d.table.nRows;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    StrCatNoSink sink;
    uint8_t nn = 0;
    int64_t len = strCatRow(st.prog, src, row, sink, &nn);
    if (len < 0) {  // the row drops out of the emit; the engine reports it
      atomicOr(d.errorFlag, kErrStrRowTooLong);
      len = 0;
      nn = 0;
    }
    lens[row] = len;
    notNull[row] = nn;
  }
}

// tile piece table in dynamic LDS, piece-major so lanes hit distinct banks:
// start[nPieces][256] i64, off[257] i64, end[nPieces][256] u32, mask[256] u8
struct CatTileTab {
  int64_t* startv;
  uint32_t* endv;
  uint8_t* maskv;
  __device__ int64_t start(int p, int r) const { return startv[p * kStrCatTile + r]; }
  __device__ int64_t end(int p, int r) const { return endv[p * kStrCatTile + r]; }
  __device__ uint32_t mask(int r) const { return maskv[r]; }
};
struct CatTileSink {
  const CatTileTab& t;
  int r;
  __device__ void put(int p, int64_t s, int64_t e) {
    t.startv[p * kStrCatTile + r] = s;
    t.endv[p * kStrCatTile + r] = (uint32_t)e;
  }
  __device__ void mask(uint32_t m) { t.maskv[r] = (uint8_t)m; }
};
static size_t catTileLdsBytes(int nPieces) {
  return (size_t)nPieces * kStrCatTile * 12 + (kStrCatTile + 1) * 8 + kStrCatTile;
}

// emit pass: a block takes 256-row tiles; each lane recomputes its row's
// piece table into LDS, then all lanes stride over the tile's contiguous
// output bytes, a dword each, so stores coalesce whatever the row lengths are
__global__ __launch_bounds__(256) void strCatEmitKernel(
    const ProjDesc* __restrict__ dp, int ci,
    const int64_t* __restrict__ outOffsets, uint8_t* __restrict__ outData) {
  __shared__ __align__(16) uint8_t stRaw[sizeof(CatStage)];
  CatStage& st = *reinterpret_cast<CatStage*>(stRaw);
  extern __shared__ __align__(16) uint8_t catLds[];
  const ProjDesc& d = *dp;
  catStageLoad(st, d, ci);
  CatDevSrc src{d, st};
  const int np = st.prog.nPieces;
  CatTileTab tab;
  tab.startv = (int64_t*)catLds;
  int64_t* off = tab.startv + np * kStrCatTile;
  tab.endv = (uint32_t*)(off + kStrCatTile + 1);
  tab.maskv = (uint8_t*)(tab.endv + np * kStrCatTile);
  const int64_t n = d.table.nRows;
  const int64_t nTiles = (n + kStrCatTile - 1) / kStrCatTile;
  const int tid = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
    const int64_t r0 = tile * kStrCatTile;
    const int T = n - r0 < kStrCatTile ? (int)(n - r0) : kStrCatTile;
    if (tid < T) {
      CatTileSink sink{tab, tid};
      uint8_t nn = 0;
      (void)strCatRow(st.prog, src, r0 + tid, sink, &nn);
    }
    for (int i = tid; i <= T; i += blockDim.x) off[i] = outOffsets[r0 + i];
    __syncthreads();
    // one aligned output word per lane and step (outData is an allocation
    // base, so w is a dword address); the tile's ragged ends store bytes
    const int64_t b0 = off[0], b1 = off[T];
    for (int64_t w = (b0 & ~(int64_t)3) + 4 * tid; w < b1;
         w += 4 * (int64_t)blockDim.x) {
      const int64_t lo = w < b0 ? b0 : w;
      const int64_t hi = w + 4 < b1 ? w + 4 : b1;
      uint32_t word = strCatWord(st.prog, src, tab, off, T, w, lo, hi);
      if (hi - lo == 4) {
        *(uint32_t*)(outData + w) = word;
      } else {
        for (int64_t g = lo; g < hi; g++)
          outData[g] = (uint8_t)(word >> (8 * (int)(g - w)));
      }
    }
    __syncthreads();
  }
}

int gxStrCatLens(const ProjDesc* devDesc, const ProjDesc& h, int catIdx,
                 int64_t* lens, uint8_t* notNull, void* stream) {
  if (h.table.nRows == 0) return 0;
  hipLaunchKernelGGL(strCatLensKernel, dim3(gridFor(h.table.nRows)), dim3(256),
                     0, (hipStream_t)stream, devDesc, catIdx, lens, notNull);
  return (int)hipGetLastError();
}

int gxStrCatEmit(const ProjDesc* devDesc, const ProjDesc& h, int catIdx,
                 const int64_t* outOffsets, uint8_t* outData, void* stream) {
  if (h.table.nRows == 0) return 0;
  hipLaunchKernelGGL(strCatEmitKernel, dim3(gridFor(h.table.nRows)), dim3(256),
                     catTileLdsBytes(h.cat[catIdx].nPieces),
                     (hipStream_t)stream, devDesc, catIdx, outOffsets, outData);
  return (int)hipGetLastError();
}

int gxProject(const ProjDesc* devDesc, const ProjDesc& h, void* stream) {
  if (h.table.nRows == 0) return 0;
  dim3 g(gridFor(h.table.nRows));
  if (h.wide)
    hipLaunchKernelGGL(projectKernel<true>, g, dim3(256), 0,
                       (hipStream_t)stream, devDesc);
  else
    hipLaunchKernelGGL(projectKernel<false>, g, dim3(256), 0,
                       (hipStream_t)stream, devDesc);
  return (int)hipGetLastError();
}

int gxPackNulls(const uint8_t* notNullBytes, uint8_t* bitmap, int64_t n,
                void* stream) {
  hipLaunchKernelGGL(packNullsKernel, dim3(gridFor((n + 7) / 8)), dim3(256), 0,
                     (hipStream_t)stream, notNullBytes, bitmap, n);
  return (int)hipGetLastError();
}

// ascending radix sort of survivor indices (restores SelectionExec's
// input-order emission after the wave-aggregated compaction)
int gxSortU32Keys(const uint32_t* in, uint32_t* out, int64_t n, void* tmp,
                  size_t* tmpBytes, void* stream) {
  return (int)hipcub::DeviceRadixSort::SortKeys(tmp, *tmpBytes, in, out,
                                                (int)n, 0, 32,
                                                (hipStream_t)stream);
}

int gxGatherNulls(const uint8_t* inBitmap, const uint32_t* idx, uint8_t* out,
                  int64_t n, void* stream) {
  hipLaunchKernelGGL(hjGatherNullsKernel, dim3(gridFor((n + 7) / 8)), dim3(256),
                     0, (hipStream_t)stream, inBitmap, idx, out, n);
  return (int)hipGetLastError();
}

int gxIotaOffsets(int64_t* p, int64_t n, void* stream) {
  hipLaunchKernelGGL(iotaI64Kernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, p, n);
  return (int)hipGetLastError();
}

int gxGatherVarlenLens(const int64_t* inOffsets, const uint32_t* idx,
                       int64_t* lens, int64_t n, void* stream) {
  hipLaunchKernelGGL(hjVarlenLensKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, inOffsets, idx, lens, n);
  return (int)hipGetLastError();
}

int gxExclusiveSumI64(const int64_t* lens, int64_t* outOffsets, int64_t n,
                      void* tmp, size_t* tmpBytes, void* stream) {
  // inclusive sum into outOffsets+1; caller zeroes outOffsets[0]
  return (int)hipcub::DeviceScan::InclusiveSum(tmp, *tmpBytes, lens,
                                               outOffsets + 1, (int)n,
                                               (hipStream_t)stream);
}

int gxGatherVarlenBytes(const uint8_t* inData, const int64_t* inOffsets,
                        const uint32_t* idx, const int64_t* outOffsets,
                        uint8_t* outData, int64_t n, void* stream) {
  hipLaunchKernelGGL(hjVarlenBytesKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, inData, inOffsets, idx, outOffsets,
                     outData, n);
  return (int)hipGetLastError();
}

// ==================================================================
// dense rank of a general varlen sort key (gx_strkey.h)
// ==================================================================

// column bytes by index into the data buffer; byte loads only, so nothing
// beyond the last byte asked for is touched
struct StrKeyBytes {
  const uint8_t* data;
  __device__ uint8_t operator()(int64_t i) const {
    return gptr<uint8_t>(data)[i];
  }
};

// one pass: effective length per row (0 under NULL, whose bytes stay
// unread) and the column's maximum
__global__ void strKeyElenKernel(const uint8_t* __restrict__ data,
                                 const int64_t* __restrict__ offsets,
                                 const uint8_t* __restrict__ nullBitmap,
                                 int64_t n, uint32_t* __restrict__ elen,
                                 uint32_t* devMax, uint32_t* errFlag) {
  uint32_t mx = 0;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
    uint32_t e = 0;
    bool isNull =
        nullBitmap && ((nullBitmap[row >> 3] >> (row & 7)) & 1) == 0;
    if (!isNull) {
      int64_t s = offsets[row];
      int64_t len = strKeyTrimLen(StrKeyBytes{data}, s, offsets[row + 1] - s);
      if (len > 0xFFFFFFFFLL) {
        atomicOr(errFlag, kErrStrRowTooLong);
        len = 0;
      }
      e = (uint32_t)len;
    }
    elen[row] = e;
    mx = e > mx ? e : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t o = __shfl_down(mx, off, 64);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(devMax, mx);
}

__global__ void strKeyComposeKernel(const uint8_t* __restrict__ data,
                                    const int64_t* __restrict__ offsets,
                                    const uint32_t* __restrict__ elen,
                                    const uint32_t* __restrict__ perm,
                                    const uint32_t* __restrict__ act,
                                    const uint32_t* __restrict__ head,
                                    int64_t m, uint32_t round,
                                    uint64_t* __restrict__ w,
                                    uint32_t* __restrict__ rowAct,
                                    uint32_t* __restrict__ headFlag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t row, hf;
    if (act) {
      uint32_t pos = act[i];
      row = perm[pos];
      hf = head[pos];
    } else {  // round 0: the strings in row order, one segment
      row = (uint32_t)i;
      hf = i == 0;
    }
    uint32_t e = elen[row];
    // offsets[row] is read only where a byte follows it
    uint64_t key = 0;
    if ((uint64_t)round * kStrKeyWin < e)
      key = strKeyWindow(StrKeyBytes{data}, offsets[row], e, round);
    w[i] = key;
    rowAct[i] = row;
    headFlag[i] = hf;
  }
}

__global__ void strKeySegKeysKernel(const uint32_t* __restrict__ seg,
                                    const uint32_t* __restrict__ order,
                                    uint64_t* __restrict__ keys, int64_t m) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x)
    keys[j] = seg[order[j]];
}

__global__ void strKeyPlaceKernel(const uint64_t* __restrict__ w,
                                  const uint32_t* __restrict__ rowAct,
                                  const uint32_t* __restrict__ order,
                                  const uint32_t* __restrict__ act,
                                  uint32_t* __restrict__ perm,
                                  uint64_t* __restrict__ wSorted, int64_t m) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    uint32_t k = order ? order[j] : (uint32_t)j;
    wSorted[j] = w[k];
    perm[act ? act[j] : (uint32_t)j] = rowAct[k];
  }
}

__global__ void strKeyRefineKernel(const uint32_t* __restrict__ seg,
                                   const uint64_t* __restrict__ wSorted,
                                   const uint32_t* __restrict__ act,
                                   uint32_t* __restrict__ head,
                                   uint8_t* __restrict__ keep, int64_t m) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += (int64_t)gridDim.x * blockDim.x) {
    if (strKeyIsHead(seg, wSorted, j)) head[act ? act[j] : (uint32_t)j] = 1;
    keep[j] = strKeyStaysActive(seg, wSorted, j, m) ? 1 : 0;
  }
}

__global__ void strKeyScatterRankKernel(const uint32_t* __restrict__ perm,
                                        const uint32_t* __restrict__ headScan,
                                        uint32_t* __restrict__ rank,
                                        int64_t n) {
  for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n;
       pos += (int64_t)gridDim.x * blockDim.x)
    rank[perm[pos]] = headScan[pos] - 1;
}

int gxStrKeyElen(const DevCol& col, int64_t n, uint32_t* elen,
                 uint32_t* devMax, uint32_t* errFlag, void* stream) {
  hipLaunchKernelGGL(strKeyElenKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, (const uint8_t*)col.data,
                     col.offsets, col.hasNulls ? col.nullBitmap : nullptr, n,
                     elen, devMax, errFlag);
  return (int)hipGetLastError();
}

int gxStrKeyCompose(const DevCol& col, const uint32_t* elen,
                    const uint32_t* perm, const uint32_t* act,
                    const uint32_t* head, int64_t m, uint32_t round,
                    uint64_t* w, uint32_t* rowAct, uint32_t* headFlag,
                    void* stream) {
  hipLaunchKernelGGL(strKeyComposeKernel, dim3(gridFor(m)), dim3(256), 0,
                     (hipStream_t)stream, (const uint8_t*)col.data,
                     col.offsets, elen, perm, act, head, m, round, w, rowAct,
                     headFlag);
  return (int)hipGetLastError();
}

int gxStrKeySegKeys(const uint32_t* seg, const uint32_t* order, uint64_t* keys,
                    int64_t m, void* stream) {
  hipLaunchKernelGGL(strKeySegKeysKernel, dim3(gridFor(m)), dim3(256), 0,
                     (hipStream_t)stream, seg, order, keys, m);
  return (int)hipGetLastError();
}

int gxStrKeyPlace(const uint64_t* w, const uint32_t* rowAct,
                  const uint32_t* order, const uint32_t* act, uint32_t* perm,
                  uint64_t* wSorted, int64_t m, void* stream) {
  hipLaunchKernelGGL(strKeyPlaceKernel, dim3(gridFor(m)), dim3(256), 0,
                     (hipStream_t)stream, w, rowAct, order, act, perm, wSorted,
                     m);
  return (int)hipGetLastError();
}

int gxStrKeyRefine(const uint32_t* seg, const uint64_t* wSorted,
                   const uint32_t* act, uint32_t* head, uint8_t* keep,
                   int64_t m, void* stream) {
  hipLaunchKernelGGL(strKeyRefineKernel, dim3(gridFor(m)), dim3(256), 0,
                     (hipStream_t)stream, seg, wSorted, act, head, keep, m);
  return (int)hipGetLastError();
}

int gxStrKeyScatterRank(const uint32_t* perm, const uint32_t* headScan,
                        uint32_t* rank, int64_t n, void* stream) {
  hipLaunchKernelGGL(strKeyScatterRankKernel, dim3(gridFor(n)), dim3(256), 0,
                     (hipStream_t)stream, perm, headScan, rank, n);
  return (int)hipGetLastError();
}

int gxInclusiveSumU32(const uint32_t* in, uint32_t* out, int64_t n, void* tmp,
                      size_t* tmpBytes, void* stream) {
  return (int)hipcub::DeviceScan::InclusiveSum(tmp, *tmpBytes, in, out, (int)n,
                                               (hipStream_t)stream);
}

int gxSelectFlaggedU32(const uint32_t* in, const uint8_t* keep, uint32_t* out,
                       uint32_t* devCount, int64_t n, void* tmp,
                       size_t* tmpBytes, void* stream) {
  if (in)
    return (int)hipcub::DeviceSelect::Flagged(tmp, *tmpBytes, in, keep, out,
                                              devCount, (int)n,
                                              (hipStream_t)stream);
  hipcub::CountingInputIterator<uint32_t> iota(0);
  return (int)hipcub::DeviceSelect::Flagged(tmp, *tmpBytes, iota, keep, out,
                                            devCount, (int)n,
                                            (hipStream_t)stream);
}

}  // namespace gxp
