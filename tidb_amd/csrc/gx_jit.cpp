// gx_jit.cpp — runtime kernel specialization via hipRTC.
//
// The interpreted fused kernel pays ~45% of its time walking the predicate
// list, the VM instruction stream and the aggregate plan per row-iteration
// (measured by ablation). A vectorized executor's classic
// answer is code generation: here the engine emits a straight-line HIP
// kernel for the exact compiled query -- literal fetch slots, literal
// parse scales and reciprocals, unrolled arithmetic, literal group-key and
// accumulator plans -- compiles it with hipRTC for gfx950 at Open, and
// launches it through hipModuleLaunchKernel. Results are identical to the
// interpreted kernel (same helpers from gx_device.h, same error flags,
// same wide/noLds retries); any compile/load failure falls back to the
// interpreted path.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "gx_common.h"
#include "gx_jit.h"

namespace gxjit {

using gxp::FusedQueryDesc;

struct JitProg {
  hipModule_t mod = nullptr;
  hipFunction_t fnNarrow = nullptr;
  hipFunction_t fnWide = nullptr;
  bool ok = false;
  int rowsPerLane = 1;  // fused-agg programs: K of the generated row loop
};

static std::map<std::string, JitProg>& cache() {
  static std::map<std::string, JitProg> c;
  return c;
}
static std::mutex cacheMu;

// directory holding gx_common.h / gx_device.h (next to this .so)
static std::string headerDir() {
  Dl_info info;
  if (dladdr((void*)&headerDir, &info) && info.dli_fname) {
    std::string p = info.dli_fname;
    size_t slash = p.rfind('/');
    if (slash != std::string::npos) return p.substr(0, slash);
  }
  return ".";
}

static const char* cmpOp(int cmp) {
  // GX_F_LT..GX_F_NE = 0..5
  switch (cmp) {
    case 0: return "<";
    case 1: return "<=";
    case 2: return ">";
    case 3: return ">=";
    case 4: return "==";
    default: return "!=";
  }
}

// declare every physical VM register once; instructions assign
static void emitVmRegs(std::ostringstream& s, int nRegs) {
  for (int r = 0; r < nRegs; r++)
    s << "  T v" << r << " = VT<WIDE>::zero(); bool n" << r
      << " = false; (void)v" << r << "; (void)n" << r << ";\n";
}

// tail of a raw decimal load into register v: a row stored at a smaller frac
// than the declared one (`frac`) scales up, a larger one is an error
static void emitDecRescale(std::ostringstream& s, const std::string& v,
                           int frac) {
  s << "    if (sc != " << frac << ") {\n"
    << "      if (sc < " << frac << ") { bool o2 = false; " << v
    << " = VT<WIDE>::scale10(" << v << ", " << frac
    << " - sc, &o2); if (o2) { atomicOr(d.errorFlag, WIDE ? kErrOverflow"
       " : kErrRetryWide); return false; } }\n"
    << "      else { atomicOr(d.errorFlag, kErrScale); return false; }\n"
    << "    }\n  }\n";
}

// emit one non-load VM instruction: the gx_vm.h value function (or the VT<>
// primitive) with literal operands. A register may be recycled as its own
// operand, so value (t2) and NULL flag (t3) are computed before either is
// assigned. Loads are the callers'.
static void emitVmOp(std::ostringstream& s, const gxp::VmIns& ins, int64_t p10,
                     const int64_t* constLo, const int64_t* constHi) {
  auto reg = [](const char* k, int r) { return k + std::to_string(r); };
  const std::string a = reg("v", ins.a), b = reg("v", ins.b),
                    c = reg("v", ins.c);
  const std::string na = reg("n", ins.a), nb = reg("n", ins.b),
                    nc = reg("n", ins.c);
  const std::string nab = na + " || " + nb;
  auto i64 = [](int64_t v) {  // literal that survives INT64_MIN
    return "(int64_t)" + std::to_string((uint64_t)v) + "ULL";
  };
  std::string nul, stmt;  // t3's initial value; statement(s) that set t2
  switch (ins.op) {
    case gxp::VM_LOAD_CONST:
      nul = "false";
      stmt = "t2 = vmConst<WIDE>(" + i64(constLo[ins.a]) + ", " +
             i64(constHi[ins.a]) + ");";
      break;
    case gxp::VM_ADD:
      nul = nab;
      stmt = "t2 = VT<WIDE>::add(" + a + ", " + b + ", &ovf);";
      break;
    case gxp::VM_SUB:
      nul = nab;
      stmt = "t2 = VT<WIDE>::sub(" + a + ", " + b + ", &ovf);";
      break;
    case gxp::VM_MUL:
      nul = nab;
      stmt = "if (!t3) t2 = VT<WIDE>::mul(" + a + ", " + b + ", &ovf);";
      break;
    case gxp::VM_SCALE_UP:
      nul = na;
      stmt = "t2 = VT<WIDE>::mul(" + a + ", VT<WIDE>::fromI64(" + i64(p10) +
             ", nullptr), &ovf);";
      break;
    case gxp::VM_TIME_EXTRACT:
      nul = na;
      stmt = "t2 = vmTimeExtract<WIDE>(" + a + ", " + std::to_string(ins.b) +
             ", &ovf);";
      break;
    case gxp::VM_CMP:
      nul = nab;
      stmt = "t2 = VT<WIDE>::fromI64(cmpResult(VT<WIDE>::cmp(" + a + ", " + b +
             "), " + std::to_string(ins.c) + ") ? 1 : 0, &ovf);";
      break;
    case gxp::VM_IF:
      nul = "false";
      stmt = "bool t = !" + na + " && VT<WIDE>::cmp(" + a +
             ", VT<WIDE>::zero()) != 0; t2 = t ? " + b + " : " + c +
             "; t3 = t ? " + nb + " : " + nc + ";";
      break;
    case gxp::VM_MAX2:
    case gxp::VM_MIN2:
      nul = nab;
      stmt = "t2 = vmSelectMinMax<WIDE>(" + a + ", " + b + ", " +
             (ins.op == gxp::VM_MAX2 ? "true" : "false") + ");";
      break;
    case gxp::VM_ABS:
      nul = na;
      stmt = "t2 = vmAbs<WIDE>(" + a + ", &ovf);";
      break;
    case gxp::VM_IFNULL:
      nul = na + " && " + nb;
      stmt = "t2 = " + na + " ? " + b + " : " + a + ";";
      break;
    case gxp::VM_ROUND_SCALE:
      nul = na;
      stmt = "if (!t3 && !vmRoundScale<WIDE>(" + a + ", " +
             std::to_string(ins.b - ins.c) + ", " + i64(p10) +
             ", &t2, &ovf, d.errorFlag)) return false;";
      break;
    case gxp::VM_DIV:
      nul = nab;
      stmt = "if (!t3 && !vmDiv<WIDE>(" + a + ", " + b + ", " +
             std::to_string(ins.c) + ", &t2, &t3, d.errorFlag)) return false;";
      break;
    default:  // not reached: compile() and compileJa() refuse such a plan
      return;
  }
  s << "  { bool t3 = " << nul << "; T t2 = VT<WIDE>::zero(); " << stmt << " "
    << reg("v", ins.dst) << " = t2; " << reg("n", ins.dst) << " = t3; }\n";
}

// Lane-replicated LDS layout of a generated kernel (first accumulation tier):
// S single keys, and per group W accumulator words in R copies each -- a
// lane adds into copy threadIdx.x & (R-1), so the lanes of one wave that
// meet the same group spread over R addresses instead of taking turns on
// one. Only what the plan uses gets a word: int128 sums two (lo, hi),
// min/max one, each count one. The copies of one word are contiguous:
// word w of copy c of slot g is acc[(g * W + w) * R + c].
struct ReplLayout {
  int R = 0, S = 0, W = 0;
  int accWord[gxp::kMaxAggs];
  int cntWord[gxp::kMaxAggs];
};

// static LDS of the single-copy layout; the replicated one stays inside it
// so a block keeps its 8-per-CU occupancy
static constexpr int kLdsBudgetBytes =
    (int)sizeof(gxp::GroupSlot) * gxp::kLdsGroups;

static bool planRepl(const FusedQueryDesc& d, ReplLayout* L) {
  int w = 0;
  for (int i = 0; i < d.nAccSlots; i++) {
    L->accWord[i] = w;
    w += d.accKind[i] == 0 ? 2 : 1;
  }
  const int nCnt = d.sharedCnt ? 1 : d.nAggs;
  for (int a = 0; a < nCnt; a++) L->cntWord[a] = w++;
  L->W = w;
  int r = 8;  // copies: 8, 16 or 32 (GX_LDS_REPL_R; default by measurement)
  if (const char* e = getenv("GX_LDS_REPL_R")) {
    int v = atoi(e);
    if (v == 8 || v == 16 || v == 32) r = v;
  }
  auto fit = [&](int copies) {  // largest power-of-two slot count, <= 16
    int sl = 16;
    while (sl > 0 && sl * (8 + copies * 8 * w) > kLdsBudgetBytes) sl >>= 1;
    return sl;
  };
  while (r > 8 && fit(r) < 8) r >>= 1;
  L->R = r;
  L->S = fit(r);
  return w > 0 && L->S >= 2;
}

int replSlots(const FusedQueryDesc& d) {
  ReplLayout L;
  return planRepl(d, &L) ? L.S : 0;
}

// emit the per-row pipeline with every plan constant baked in; L selects the
// lane-replicated LDS layout
static void emitRowPipe(std::ostringstream& s, const FusedQueryDesc& d,
                        const ReplLayout* L) {
  s << "template <bool WIDE>\n"
       "__device__ __forceinline__ bool rowPipe(const FusedQueryDesc& d, "
       "int64_t row, const RawT& raw, "
    << (L ? "Lds3U64* lkeys, Lds3U64* lacc" : "Lds3GroupSlot* lds")
    << ", uint64_t* mySel) {\n"
       "  using T = typename VT<WIDE>::T;\n"
       "  bool ovf = false; (void)ovf;\n";
  // registers are RECYCLED by the plan compiler
  emitVmRegs(s, d.nVmRegs);
  // ---- predicates (literal) ----
  for (int p = 0; p < d.nPreds; p++) {
    const gxp::PredDesc& pd = d.preds[p];
    const gxp::DevCol& c = d.table.cols[pd.col];
    if (pd.kind == gxp::PRED_IS_NULL) {  // no null-reject: null IS the result
      s << "  if (!evalSimplePred(d.table, d.preds[" << p
        << "], d.preds[" << p << "].strC, d.preds[" << p
        << "].strCLen, row)) return true;\n";
      continue;
    }
    if (c.hasNulls)
      s << "  if (colIsNull(d.table.cols[" << pd.col << "], row)) return true;\n";
    if (pd.kind == gxp::PRED_TIME_CMP_CONST) {
      s << "  if (!((raw.get(" << pd.slot << ").x & ~0xFULL) " << cmpOp(pd.cmp)
        << " " << (pd.constU64 & ~0xFULL) << "ULL)) return true;\n";
    } else if (pd.kind == gxp::PRED_I64_CMP_CONST) {
      s << "  if (!((int64_t)raw.get(" << pd.slot << ").x " << cmpOp(pd.cmp)
        << " (int64_t)" << (int64_t)pd.constU64 << "LL)) return true;\n";
    } else if (pd.kind == gxp::PRED_DEC_CMP_CONST && pd.slot >= 0 &&
               d.fetch[pd.slot].kind == gxp::FETCH_UNITS8) {
      // proven column: the slot holds int64 units at the const's scale
      s << "  if (!((int64_t)raw.get(" << pd.slot << ").x " << cmpOp(pd.cmp)
        << " (int64_t)" << (int64_t)pd.constU64 << "LL)) return true;\n";
    } else if (pd.kind == gxp::PRED_DEC_CMP_CONST) {
      s << "  { T u; int sc;\n"
           "    if (!loadDecimalUnits<WIDE>((const uint8_t*)d.table.cols["
        << pd.col << "].data + row * 40, &u, &sc, d.errorFlag)) return false;\n"
           "    if (!(VT<WIDE>::cmp(u, VT<WIDE>::fromI64((int64_t)"
        << (int64_t)pd.constU64 << "LL, nullptr)) " << cmpOp(pd.cmp)
        << " 0)) return true; }\n";
    } else {  // string EQ/LIKE: shared interpreted helper (cold conjunct)
      s << "  if (!evalSimplePred(d.table, d.preds[" << p
        << "], d.preds[" << p << "].strC, d.preds[" << p
        << "].strCLen, row)) return true;\n";
    }
  }
  s << "  (*mySel)++;\n";
  // ---- straight-line VM ----
  for (int i = 0; i < d.nIns; i++) {
    const gxp::VmIns& ins = d.ins[i];
    std::string v = "v" + std::to_string(ins.dst);
    std::string nv = "n" + std::to_string(ins.dst);
    switch (ins.op) {
      case gxp::VM_LOAD_DEC: {
        const gxp::DevCol& c = d.table.cols[ins.a];
        s << "  " << v << " = VT<WIDE>::zero(); " << nv << " = false;\n";
        if (c.hasNulls)
          s << "  " << nv << " = colIsNull(d.table.cols[" << ins.a
            << "], row);\n";
        if (d.fetch[ins.c].kind == gxp::FETCH_UNITS8) {
          // proven column: units at scale ins.b straight from the slot
          s << "  if (!" << nv << ") " << v
            << " = VT<WIDE>::fromI64((int64_t)raw.get(" << ins.c
            << ").x, nullptr);\n";
          break;
        }
        s << "  if (!" << nv << ") { int sc;\n"
          << "    if (!parseDecimalRaw<WIDE>(raw.get(" << ins.c << "), &" << v
          << ", &sc, d.errorFlag, " << ins.b << ", " << d.insP10[i] << "LL, "
          << d.insMagic[i] << "ULL)) return false;\n";
        emitDecRescale(s, v, ins.b);
        break;
      }
      case gxp::VM_LOAD_I64: {
        const gxp::DevCol& c = d.table.cols[ins.a];
        s << "  " << nv << " = false;\n";
        if (c.hasNulls)
          s << "  " << nv << " = colIsNull(d.table.cols[" << ins.a
            << "], row);\n";
        s << "  " << v << " = " << nv
          << " ? VT<WIDE>::zero() : VT<WIDE>::fromI64((int64_t)raw.get("
          << ins.c << ").x, &ovf);\n";
        break;
      }
      case gxp::VM_LIKE: {
        // value-context LIKE: the shared matcher over the desc's pattern
        // table (loads at use; NULL string -> NULL)
        const gxp::DevCol& c = d.table.cols[ins.a];
        s << "  { bool t3 = "
          << (c.hasNulls ? "colIsNull(d.table.cols[" + std::to_string(ins.a) +
                               "], row)"
                         : std::string("false"))
          << ";\n    " << v << " = VT<WIDE>::fromI64(!t3 && likeColMatch("
          << "d.table.cols[" << ins.a << "], d.likePats[" << ins.b
          << "], row) != " << (ins.c != 0 ? "true" : "false")
          << " ? 1 : 0, &ovf); " << nv << " = t3; }\n";
        break;
      }
      default:
        emitVmOp(s, ins, d.insP10[i], d.constLo, d.constHi);
        break;
    }
  }
  s << "  if (ovf) { atomicOr(d.errorFlag, WIDE ? kErrOverflow : "
       "kErrRetryWide); return false; }\n";
  // ---- group key (literal kinds/slots) ----
  s << "  uint64_t key = 0;\n";
  for (int k = 0; k < d.gkey.nCols; k++) {
    const gxp::DevCol& c = d.table.cols[d.gkey.col[k]];
    s << "  { uint32_t lane;\n";
    if (c.hasNulls)
      s << "    if (colIsNull(d.table.cols[" << d.gkey.col[k]
        << "], row)) lane = 0xFF000000u; else\n";
    if (d.gkey.kind[k] == 2) {
      if (d.gkey.rawSlot[k] >= 0)
        s << "    { uint8_t b = (uint8_t)(raw.get(" << d.gkey.rawSlot[k]
          << ").y >> " << (8 * k) << ");\n";
      else
        s << "    { uint8_t b = gptr<uint8_t>(d.table.cols[" << d.gkey.col[k]
          << "].data)[row];\n";
      s << "      lane = b == ' ' ? 0u : ((1u << 24) | b); }\n";
    } else {  // kind 1: small i64
      s << "    { int64_t gv = (int64_t)raw.get(" << d.gkey.slot[k]
        << ").x;\n"
           "      if (gv < 0 || gv > 0x7FFFFFFF) { atomicOr(d.errorFlag, "
           "kErrBadKey); return false; }\n"
           "      lane = (uint32_t)gv; }\n";
    }
    s << "    key |= (uint64_t)lane << " << (32 * k) << "; }\n";
  }
  if (d.gkey.nCols == 0) s << "  key = 0;\n";
  s << "  if (key == kEmptyKey) key = kEmptyKey - 1;\n";
  // ---- group probe + accumulate (literal plan; runtime noLds retry) ----
  if (L) {
    // replicated tier: a block that meets more keys than the small table
    // holds asks for the single-copy layout (kErrLdsSmall)
    s << "  if (!d.noLds) {\n"
         "    uint32_t slot = (uint32_t)(splitmix64(key) & (kReplSlots - 1));\n"
         // the small constant bound invites full unrolling of a loop that
         // ends at its first probe: 8 VGPRs for nothing
         "    _Pragma(\"nounroll\") for (int probe = 0;; probe++) {\n"
         "      if (probe >= kReplSlots) { atomicOr(d.errorFlag, kErrLdsSmall); "
         "return false; }\n"
         "      uint64_t cur = lkeys[slot];\n"
         "      if (cur == key) break;\n"
         "      if (cur == kEmptyKey) {\n"
         "        uint64_t prev = lds3WordCas(&lkeys[slot], kEmptyKey, key);\n"
         "        if (prev == kEmptyKey || prev == key) break;\n"
         "      }\n"
         "      slot = (slot + 1) & (kReplSlots - 1);\n"
         "    }\n"
         "    Lds3U64* t = lacc + slot * (kReplWords * kReplCopies);\n";
    auto word = [&](int w) {
      return "t + " + std::to_string(w) + " * kReplCopies";
    };
    if (d.sharedCnt) s << "    lds3WordAdd(" << word(L->cntWord[0]) << ", 1);\n";
    for (int sIdx = 0; sIdx < d.nAccSlots; sIdx++) {
      if (d.accKind[sIdx] == 0) {
        s << "    if (!n" << d.accReg[sIdx] << ") lds3WordAddAcc("
          << word(L->accWord[sIdx]) << ", " << word(L->accWord[sIdx] + 1)
          << ", VT<WIDE>::toAcc(v" << d.accReg[sIdx] << "));\n";
      } else {
        s << "    if (!n" << d.accReg[sIdx] << ") { Int128 mv = "
             "VT<WIDE>::toAcc(v" << d.accReg[sIdx] << ");\n"
          << "      bool fits = (mv.hi == 0 && (int64_t)mv.lo >= 0) || "
             "(mv.hi == -1 && (int64_t)mv.lo < 0);\n"
          << "      if (WIDE && !fits) { atomicOr(d.errorFlag, kErrOverflow); "
             "return false; }\n"
          << "      uint64_t enc = biasI64((int64_t)mv.lo);\n"
          << "      lds3WordMax(" << word(L->accWord[sIdx]) << ", "
          << (d.accKind[sIdx] == 2 ? "~enc" : "enc") << "); }\n";
      }
    }
    if (!d.sharedCnt) {
      for (int a = 0; a < d.nAggs; a++) {
        const gxp::AggDesc& ad = d.aggs[a];
        if (ad.fr >= 0) continue;
        if (ad.srcReg >= 0)
          s << "    if (!n" << ad.srcReg << ") lds3WordAdd("
            << word(L->cntWord[a]) << ", 1);\n";
        else
          s << "    lds3WordAdd(" << word(L->cntWord[a]) << ", 1);\n";
      }
    }
    s << "    return true;\n  }\n";
  } else {
    s << "  if (!d.noLds) {\n"
         "    uint32_t slot = (uint32_t)(splitmix64(key) & (kLdsGroups - 1));\n"
         "    for (int probe = 0;; probe++) {\n"
         "      if (probe >= kLdsGroups) { atomicOr(d.errorFlag, kErrLdsFull); "
         "return false; }\n"
         "      uint64_t cur = lds[slot].key;\n"
         "      if (cur == key) break;\n"
         "      if (cur == kEmptyKey) {\n"
         "        uint64_t prev = lds3CasKey(&lds[slot], kEmptyKey, key);\n"
         "        if (prev == kEmptyKey || prev == key) break;\n"
         "      }\n"
         "      slot = (slot + 1) & (kLdsGroups - 1);\n"
         "    }\n"
         "    Lds3GroupSlot* t = &lds[slot];\n";
    if (d.sharedCnt) s << "    lds3AccumCnt(t, 0, 1);\n";
    for (int sIdx = 0; sIdx < d.nAccSlots; sIdx++) {
      if (d.accKind[sIdx] == 0) {
        s << "    if (!n" << d.accReg[sIdx] << ") lds3AccumAcc(t, " << sIdx
          << ", VT<WIDE>::toAcc(v" << d.accReg[sIdx] << "));\n";
      } else {
        s << "    if (!n" << d.accReg[sIdx] << ") { Int128 mv = "
             "VT<WIDE>::toAcc(v" << d.accReg[sIdx] << ");\n"
          << "      bool fits = (mv.hi == 0 && (int64_t)mv.lo >= 0) || "
             "(mv.hi == -1 && (int64_t)mv.lo < 0);\n"
          << "      if (WIDE && !fits) { atomicOr(d.errorFlag, kErrOverflow); "
             "return false; }\n"
          << "      uint64_t enc = biasI64((int64_t)mv.lo);\n"
          << "      lds3AccumMax(t, " << sIdx << ", "
          << (d.accKind[sIdx] == 2 ? "~enc" : "enc") << "); }\n";
      }
    }
    if (!d.sharedCnt) {
      for (int a = 0; a < d.nAggs; a++) {
        const gxp::AggDesc& ad = d.aggs[a];
        if (ad.fr >= 0) continue;
        if (ad.srcReg >= 0)
          s << "    if (!n" << ad.srcReg << ") lds3AccumCnt(t, " << a
            << ", 1);\n";
        else
          s << "    lds3AccumCnt(t, " << a << ", 1);\n";
      }
    }
    s << "    return true;\n  }\n";
  }
  // global-direct path
  s << "  { uint32_t gmask = (1u << d.globalGroupsLog2) - 1;\n"
       "    uint32_t slot = (uint32_t)(splitmix64(key) & gmask);\n"
       "    for (uint32_t probe = 0;; probe++) {\n"
       "      if (probe > gmask) { atomicOr(d.errorFlag, "
       "kErrGlobalFull); return false; }\n"
       "      uint64_t cur = d.globalTable[slot].key;\n"
       "      if (cur == key) break;\n"
       "      if (cur == kEmptyKey) {\n"
       "        uint64_t prev = atomicCAS((unsigned long long*)&d.globalTable"
       "[slot].key, (unsigned long long)kEmptyKey, (unsigned long long)key);\n"
       "        if (prev == kEmptyKey || prev == key) break;\n"
       "      }\n"
       "      slot = (slot + 1) & gmask;\n"
       "    }\n"
       "    GroupSlot* t = &d.globalTable[slot];\n";
  if (d.sharedCnt) s << "    accumInto(t, 0, Int128{0, 0}, 1);\n";
  for (int sIdx = 0; sIdx < d.nAccSlots; sIdx++) {
    if (d.accKind[sIdx] == 0) {
      s << "    if (!n" << d.accReg[sIdx] << ") accumInto(t, " << sIdx
        << ", VT<WIDE>::toAcc(v" << d.accReg[sIdx] << "), 0);\n";
    } else {
      s << "    if (!n" << d.accReg[sIdx] << ") { Int128 mv = "
           "VT<WIDE>::toAcc(v" << d.accReg[sIdx] << ");\n"
        << "      bool fits = (mv.hi == 0 && (int64_t)mv.lo >= 0) || "
           "(mv.hi == -1 && (int64_t)mv.lo < 0);\n"
        << "      if (WIDE && !fits) { atomicOr(d.errorFlag, kErrOverflow); "
           "return false; }\n"
        << "      uint64_t enc = biasI64((int64_t)mv.lo);\n"
        << "      accumMax(t, " << sIdx << ", "
        << (d.accKind[sIdx] == 2 ? "~enc" : "enc") << "); }\n";
    }
  }
  if (!d.sharedCnt) {
    for (int a = 0; a < d.nAggs; a++) {
      const gxp::AggDesc& ad = d.aggs[a];
      if (ad.fr >= 0) continue;
      if (ad.srcReg >= 0)
        s << "    if (!n" << ad.srcReg << ") accumInto(t, " << a << ", "
             "Int128{0, 0}, 1);\n";
      else
        s << "    accumInto(t, " << a << ", Int128{0, 0}, 1);\n";
    }
  }
  s << "  }\n  return true;\n}\n\n";
}

// width of the units column behind a FETCH_UNITS8 slot (8 unless narrowed)
static int unitsWidth(const FusedQueryDesc& d, int col) {
  const int w = d.table.cols[col].unitsWidth;
  return w == 1 || w == 2 || w == 4 ? w : 8;
}

// Rows a lane takes per load in the generated kernel: K
// consecutive rows from a K-aligned row, each stream fetched with ONE load of
// K * width bytes. Only where every fetch slot has a blocked form: units of
// any width, 8 B columns and the dense char(1) pair; a plan with an offsets
// pair or a 40 B decimal slot keeps one row per lane.
int progRowsPerLane(const JitProg* prog) { return prog ? prog->rowsPerLane : 1; }

int rowsPerLane(const FusedQueryDesc& d) {
  int k = 4;
  if (const char* e = getenv("GX_ROWS_PER_LANE")) k = atoi(e);
  if (k != 2 && k != 4) return 1;
  bool any = false;
  for (int f = 0; f < d.nFetch; f++) {
    const int kind = d.fetch[f].kind;
    if (kind == gxp::FETCH_B1) continue;
    if (kind == gxp::FETCH_OFFSETS || kind == gxp::FETCH_DEC16) return 1;
    any = true;
  }
  return any ? k : 1;
}

// one packed stream of the blocked fetch: K values of `width` bytes
struct BlkStream {
  std::string name;  // member of BlkT
  std::string base;  // column buffer expression
  int width;
};

// the j-th 32-bit word of a stream's K-row load
static std::string blkWord(const BlkStream& st, int K, int j) {
  const int bytes = K * st.width;
  static const char* xyzw[] = {".x", ".y", ".z", ".w"};
  if (bytes <= 4) return "(uint32_t)b." + st.name;
  if (bytes <= 16) return "b." + st.name + xyzw[j];
  return "b." + st.name + (j < 4 ? "" : "_h") + xyzw[j & 3];
}

static const char* blkType(int bytes) {
  return bytes == 2 ? "uint16_t" : bytes == 4 ? "uint32_t"
         : bytes == 8 ? "uint2" : "uint4";
}

// Blocked form of emitFetch: BlkT holds one K-row load per stream, fetchBlk
// issues them, unpackBlk<k> rebuilds row k's raw slots -- the same slot
// values the one-row fetchGen produces, so rowPipe does not change.
static void emitFetchBlk(std::ostringstream& s, const FusedQueryDesc& d,
                         int K) {
  std::vector<BlkStream> streams;
  // per fetch slot: index of its value stream and of its char streams
  int valueOf[gxp::kMaxFetch], chr0[gxp::kMaxFetch], chr1[gxp::kMaxFetch];
  for (int f = 0; f < d.nFetch; f++) {
    const gxp::FetchDesc& fd = d.fetch[f];
    valueOf[f] = chr0[f] = chr1[f] = -1;
    if (fd.kind == gxp::FETCH_B1) continue;
    const std::string n = "s" + std::to_string(f);
    auto col = [](int c, const char* m) {
      return "t.cols[" + std::to_string(c) + "]." + m;
    };
    if (fd.kind == gxp::FETCH_8B || fd.kind == gxp::FETCH_8B_CHAR2) {
      valueOf[f] = (int)streams.size();
      streams.push_back({n, col(fd.col, "data"), 8});
    } else if (fd.kind == gxp::FETCH_UNITS8) {
      valueOf[f] = (int)streams.size();
      streams.push_back({n, col(fd.col, "units"), unitsWidth(d, fd.col)});
    }
    if (fd.kind == gxp::FETCH_8B_CHAR2 || fd.kind == gxp::FETCH_CHAR2) {
      chr0[f] = (int)streams.size();
      streams.push_back({n + "_c0", col(fd.ldsOff & 0xFF, "data"), 1});
      if (((fd.ldsOff >> 16) & 0xFF) > 1) {
        chr1[f] = (int)streams.size();
        streams.push_back({n + "_c1", col((fd.ldsOff >> 8) & 0xFF, "data"), 1});
      }
    }
  }
  s << "constexpr int kRowsPerLane = " << K << ";\nstruct BlkT {\n";
  for (const BlkStream& st : streams) {
    const int bytes = K * st.width;
    s << "  " << blkType(bytes) << " " << st.name;
    if (bytes == 32) s << ", " << st.name << "_h";
    s << ";\n";
  }
  s << "};\n"
       "// every K-row load is aligned when its column buffer is\n"
       "__device__ __forceinline__ bool blkAligned(const DevTable& t) {\n"
       "  uintptr_t a = 0;\n";
  for (const BlkStream& st : streams)
    s << "  a |= (uintptr_t)" << st.base << ";\n";
  s << "  return (a & 15) == 0;\n}\n"
       "__device__ __forceinline__ void fetchBlk(const DevTable& t, "
       "int64_t row, BlkT& b) {\n";
  for (const BlkStream& st : streams) {
    const int bytes = K * st.width;
    s << "  b." << st.name << " = blkLoad<" << blkType(bytes) << ">("
      << st.base << ", row, " << st.width << ");\n";
    if (bytes == 32)
      s << "  b." << st.name << "_h = blkLoad<uint4>(" << st.base << ", row + "
        << K / 2 << ", " << st.width << ");\n";
  }
  s << "}\n";
  auto chr = [&](const BlkStream& st, int k) {
    return "((" + blkWord(st, K, k >> 2) + " >> " + std::to_string(8 * (k & 3)) +
           ") & 0xFFu)";
  };
  for (int k = 0; k < K; k++) {
    s << "__device__ __forceinline__ void unpackBlk" << k
      << "(const BlkT& b, RawT& r) {\n";
    for (int f = 0; f < d.nFetch; f++) {
      const gxp::FetchDesc& fd = d.fetch[f];
      if (fd.kind == gxp::FETCH_B1) continue;
      const std::string m = "r.s" + std::to_string(f);
      s << "  " << m << ".x = ";
      if (valueOf[f] < 0) {
        s << "0;\n";
      } else {
        const BlkStream& st = streams[valueOf[f]];
        s << "(uint64_t)";
        if (st.width == 1)
          s << "unitsUnpack1(" << blkWord(st, K, k >> 2) << ", " << (k & 3)
            << ");\n";
        else if (st.width == 2)
          s << "unitsUnpack2(" << blkWord(st, K, k >> 1) << ", " << (k & 1)
            << ");\n";
        else if (st.width == 4)
          s << "unitsUnpack4(" << blkWord(st, K, k) << ");\n";
        else
          s << "unitsUnpack8(" << blkWord(st, K, 2 * k) << ", "
            << blkWord(st, K, 2 * k + 1) << ");\n";
      }
      s << "  " << m << ".y = ";
      if (chr0[f] < 0) {
        s << "0;\n";
      } else {
        s << "(uint64_t)(" << chr(streams[chr0[f]], k);
        if (chr1[f] >= 0) s << " | (" << chr(streams[chr1[f]], k) << " << 8)";
        s << ");\n";
      }
    }
    s << "}\n";
  }
  s << "\n";
}

// run the K rows of one lane's block through rowPipe: from the block's loads
// when it lies inside [begin, end) whole, else (the fewer than K rows at the
// end of the table, or a column buffer that is not 16 B aligned) row by row
// through the one-row fetch
static void emitRunBlk(std::ostringstream& s, int K, bool repl) {
  const char* ldsParams =
      repl ? "Lds3U64* lkeys, Lds3U64* lacc" : "Lds3GroupSlot* lds";
  const char* ldsArgs = repl ? "lkeys, lacc" : "lds";
  s << "template <bool WIDE>\n"
       "__device__ __forceinline__ bool runBlk(const FusedQueryDesc& d, "
       "int64_t row, int64_t end, bool vec, const BlkT& b, "
    << ldsParams << ", uint64_t* mySel) {\n"
       "  RawT r;\n"
       "  if (vec && row + kRowsPerLane <= end) {\n";
  for (int k = 0; k < K; k++)
    s << "    unpackBlk" << k << "(b, r);\n"
      << "    if (!rowPipe<WIDE>(d, row + " << k << ", r, " << ldsArgs
      << ", mySel)) return false;\n";
  s << "    return true;\n  }\n"
       "  for (int64_t x = row; x < end && x < row + kRowsPerLane; x++) {\n"
       "    fetchGen(d.table, x, r);\n"
       "    if (!rowPipe<WIDE>(d, x, r, " << ldsArgs << ", mySel)) return false;\n"
       "  }\n  return true;\n}\n\n";
}

// literal fetch of every raw slot for one row
static void emitFetch(std::ostringstream& s, const FusedQueryDesc& d) {
  s << "__device__ __forceinline__ void fetchGen(const DevTable& t, "
       "int64_t row, RawT& r) {\n";
  for (int f = 0; f < d.nFetch; f++) {
    const gxp::FetchDesc& fd = d.fetch[f];
    if (fd.kind == gxp::FETCH_B1) continue;  // staged-variant-only stream
    std::string m = "r.s" + std::to_string(f);
    if (fd.kind == gxp::FETCH_8B) {
      s << "  " << m << ".x = gptr<uint64_t>(t.cols[" << fd.col
        << "].data)[row]; " << m << ".y = 0;\n";
    } else if (fd.kind == gxp::FETCH_8B_CHAR2 || fd.kind == gxp::FETCH_CHAR2) {
      if (fd.kind == gxp::FETCH_8B_CHAR2)
        s << "  " << m << ".x = gptr<uint64_t>(t.cols[" << fd.col
          << "].data)[row];\n";
      else
        s << "  " << m << ".x = 0;\n";
      s << "  { uint64_t ch = (uint64_t)gptr<uint8_t>(t.cols["
        << (fd.ldsOff & 0xFF) << "].data)[row];\n";
      if (((fd.ldsOff >> 16) & 0xFF) > 1)
        s << "    ch |= (uint64_t)gptr<uint8_t>(t.cols["
          << ((fd.ldsOff >> 8) & 0xFF) << "].data)[row] << 8;\n";
      s << "    " << m << ".y = ch; }\n";
    } else if (fd.kind == gxp::FETCH_DEC16) {
      s << "  { const uint8_t* p = (const uint8_t*)t.cols[" << fd.col
        << "].data + row * 40;\n"
        << "    " << m << ".x = *gptr<uint64_t>(p); " << m
        << ".y = *gptr<uint64_t>(p + 8); }\n";
    } else if (fd.kind == gxp::FETCH_UNITS8) {
      // the proven width as a literal typed load, sign-extended to the slot
      s << "  " << m << ".x = (uint64_t)(int64_t)gptr<int"
        << 8 * unitsWidth(d, fd.col) << "_t>(t.cols[" << fd.col
        << "].units)[row]; " << m << ".y = 0;\n";
    } else {  // FETCH_OFFSETS
      s << "  " << m << ".x = (uint64_t)gptr<int64_t>(t.cols[" << fd.col
        << "].offsets)[row]; " << m << ".y = (uint64_t)gptr<int64_t>(t.cols["
        << fd.col << "].offsets)[row + 1];\n";
    }
  }
  s << "}\n\n";
}

static std::string genSource(const FusedQueryDesc& d, bool repl, bool occ8) {
  ReplLayout layout;
  const ReplLayout* L = repl && planRepl(d, &layout) ? &layout : nullptr;
  // raw slot bound (same rule as the interpreted launcher)
  int maxSlot = -1;
  for (int f = 0; f < d.nFetch; f++)
    if (d.fetch[f].kind != gxp::FETCH_B1 && f > maxSlot) maxSlot = f;
  const char* rawT = maxSlot < 5 ? "RawState5" : "RawState";

  std::ostringstream s;
  s << "#include \"gx_common.h\"\n#include \"gx_device.h\"\n"
       "using namespace gxp;\nusing RawT = " << rawT << ";\n\n";
  if (L)
    s << "constexpr int kReplSlots = " << L->S << ", kReplCopies = " << L->R
      << ", kReplWords = " << L->W << ";\n\n";
  const int K = rowsPerLane(d);
  emitFetch(s, d);
  if (K > 1) emitFetchBlk(s, d, K);
  emitRowPipe(s, d, L);
  if (K > 1) emitRunBlk(s, K, L != nullptr);
  // kernel wrapper: same prologue/pipeline/epilogue as fusedAggKernel
  s << R"(
template <bool WIDE>
__device__ __forceinline__ void kernBody(const FusedQueryDesc* __restrict__ dp) {
  const FusedQueryDesc& d = *dp;
  // any error flag dooms the pass: late blocks bail before fetching
  if (__hip_atomic_load(d.errorFlag, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT))
    return;
  bool failed = false;
)";
  if (L)
    s << R"(  __shared__ uint64_t ldsKeys[kReplSlots];
  __shared__ uint64_t ldsAcc[kReplSlots * kReplWords * kReplCopies];
  Lds3U64* lkeys = (Lds3U64*)ldsKeys;
  // this lane's copy: folded into the base once, not per row
  Lds3U64* lacc = (Lds3U64*)ldsAcc + (threadIdx.x & (kReplCopies - 1));
  for (int i = threadIdx.x; i < kReplSlots; i += blockDim.x)
    ldsKeys[i] = kEmptyKey;
  for (int i = threadIdx.x; i < kReplSlots * kReplWords * kReplCopies;
       i += blockDim.x)
    ldsAcc[i] = 0;
)";
  else
    s << R"(  __shared__ GroupSlot lds[kLdsGroups];
  Lds3GroupSlot* lds3 = (Lds3GroupSlot*)lds;
  for (int i = threadIdx.x; i < kLdsGroups; i += blockDim.x) {
    lds[i].key = kEmptyKey;
    for (int a = 0; a < kMaxAggs; a++) {
      lds[i].accLo[a] = 0;
      lds[i].accHi[a] = 0;
      lds[i].cnt[a] = 0;
    }
  }
)";
  const char* ldsArgs = L ? "lkeys, lacc" : "lds3";
  s << R"(  __syncthreads();
  int64_t n = d.table.nRows;
  int64_t per = (n + gridDim.x - 1) / gridDim.x;
)";
  if (K > 1)  // every block begins at a K-aligned row
    s << "  per = (per + kRowsPerLane - 1) / kRowsPerLane * kRowsPerLane;\n";
  s << R"(  int64_t begin = (int64_t)blockIdx.x * per;
  int64_t end = begin + per;
  if (end > n) end = n;
  uint64_t mySel = 0;
)";
  if (K > 1)
    // two-deep pipeline over blocks of K rows per lane
    s << R"(  {
    const bool vec = blkAligned(d.table);
    const int64_t stride = (int64_t)blockDim.x * kRowsPerLane;
    int64_t row = begin + (int64_t)threadIdx.x * kRowsPerLane;
    BlkT blkA, blkB;
    if (vec && row + kRowsPerLane <= end) fetchBlk(d.table, row, blkA);
    for (; row < end && !failed; row += 2 * stride) {
      const int64_t rB = row + stride;
      if (vec && rB + kRowsPerLane <= end) fetchBlk(d.table, rB, blkB);
      if (!runBlk<WIDE>(d, row, end, vec, blkA, )" << ldsArgs << R"(, &mySel)) { failed = true; break; }
      const int64_t rA2 = row + 2 * stride;
      if (vec && rA2 + kRowsPerLane <= end) fetchBlk(d.table, rA2, blkA);
      if (rB < end && !runBlk<WIDE>(d, rB, end, vec, blkB, )" << ldsArgs << R"(, &mySel)) failed = true;
    }
  }
)";
  else
    s << R"(  {
    const int64_t stride = blockDim.x;
    int64_t row = begin + threadIdx.x;
    RawT rawA, rawB;
    if (row < end) fetchGen(d.table, row, rawA);
    for (; row < end && !failed; row += 2 * stride) {
      const int64_t rB = row + stride;
      if (rB < end) fetchGen(d.table, rB, rawB);
      if (!rowPipe<WIDE>(d, row, rawA, )" << ldsArgs << R"(, &mySel)) { failed = true; break; }
      const int64_t rA2 = row + 2 * stride;
      if (rA2 < end) fetchGen(d.table, rA2, rawA);
      if (rB < end && !rowPipe<WIDE>(d, rB, rawB, )" << ldsArgs << R"(, &mySel)) failed = true;
    }
  }
)";
  s << R"(  if (d.selCount) {
    uint64_t total = mySel;
    for (int off = 32; off > 0; off >>= 1)
      total += __shfl_down(total, off, 64);
    if ((threadIdx.x & 63) == 0 && total)
      atomicAdd((unsigned long long*)d.selCount, (unsigned long long)total);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < )" << (L ? "kReplSlots" : "kLdsGroups")
    << R"(; i += blockDim.x) {
    uint64_t key = )" << (L ? "ldsKeys[i]" : "lds[i].key") << R"(;
    if (key == kEmptyKey) continue;
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
)";
  if (L) {
    // fold the copies of each word (sums as 128-bit values, counts add,
    // biased min/max takes the maximum: zero is the identity of all three),
    // then ONE global update per word, as the single-copy flush does
    s << "    const uint64_t* g = &ldsAcc[i * (kReplWords * kReplCopies)];\n";
    for (int sIdx = 0; sIdx < d.nAccSlots; sIdx++) {
      const int w = L->accWord[sIdx];
      if (d.accKind[sIdx] != 0) {
        s << "    { uint64_t m = 0;\n"
             "      for (int c = 0; c < kReplCopies; c++) { uint64_t x = g["
          << w << " * kReplCopies + c]; if (x > m) m = x; }\n"
             "      accumMax(&d.globalTable[slot], " << sIdx << ", m); }\n";
      } else {
        s << "    { Int128 v = {0, 0};\n"
             "      for (int c = 0; c < kReplCopies; c++) {\n"
             "        uint64_t lo = g[" << w << " * kReplCopies + c];\n"
             "        uint64_t nl = v.lo + lo;\n"
             "        v.hi = (int64_t)((uint64_t)v.hi + g[" << (w + 1)
          << " * kReplCopies + c] + (nl < lo ? 1 : 0));\n"
             "        v.lo = nl;\n"
             "      }\n"
             "      accumInto(&d.globalTable[slot], " << sIdx << ", v, 0); }\n";
      }
    }
    const int nCnt = d.sharedCnt ? 1 : d.nAggs;
    for (int a = 0; a < nCnt; a++)
      s << "    { uint64_t c2 = 0;\n"
           "      for (int c = 0; c < kReplCopies; c++) c2 += g["
        << L->cntWord[a] << " * kReplCopies + c];\n"
           "      accumInto(&d.globalTable[slot], " << a
        << ", Int128{0, 0}, (int64_t)c2); }\n";
  } else {
    s << R"(    for (int s2 = 0; s2 < d.nAccSlots; s2++) {
      if (d.accKind[s2] != 0) {
        accumMax(&d.globalTable[slot], s2, lds[i].accLo[s2]);
        continue;
      }
      Int128 v = {lds[i].accLo[s2], lds[i].accHi[s2]};
      accumInto(&d.globalTable[slot], s2, v, 0);
    }
    int nCnt = d.sharedCnt ? 1 : d.nAggs;
    for (int a = 0; a < nCnt; a++)
      accumInto(&d.globalTable[slot], a, Int128{0, 0}, lds[i].cnt[a]);
)";
  }
  s << R"(  }
}

extern "C" __global__ void __launch_bounds__(256) )"
    << (occ8 ? "__attribute__((amdgpu_waves_per_eu(8))) " : "")
    << R"(genq_narrow(const FusedQueryDesc* __restrict__ dp) {
  kernBody<false>(dp);
}
extern "C" __global__ void __launch_bounds__(256) genq_wide(const FusedQueryDesc* __restrict__ dp) {
  kernBody<true>(dp);
}
)";
  return s.str();
}

// The replicated narrow kernel asks for 8 waves per SIMD (<= 64 VGPRs, what
// the single-copy kernels of the measured plans get on their own): its second
// LDS base and copy offset cost the wide-projection plan 6 VGPRs and one wave
// otherwise. compile() drops the request when it makes the kernel spill.
// The K-row form holds two blocks of loads in registers and is known to
// spill at 64 VGPRs, so only the one-row form makes the request.
static bool wantOcc8(const FusedQueryDesc& d, bool repl) {
  return repl && rowsPerLane(d) == 1;
}

std::string generateSource(const FusedQueryDesc& d, bool repl) {
  return genSource(d, repl, wantOcc8(d, repl));
}

// hipRTC-compile `src` for gfx950 and load the code object; nullptr (and
// whyNot) on any failure
static hipModule_t compileModule(const std::string& src, const char* name,
                                 std::string* whyNot) {
  hiprtcProgram rp;
  if (hiprtcCreateProgram(&rp, src.c_str(), name, 0, nullptr, nullptr) !=
      HIPRTC_SUCCESS) {
    if (whyNot) *whyNot = "hiprtcCreateProgram failed";
    return nullptr;
  }
  std::string inc = "-I" + headerDir();
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                        inc.c_str()};
  if (hiprtcCompileProgram(rp, 4, opts) != HIPRTC_SUCCESS) {
    if (whyNot) {
      size_t lsz = 0;
      hiprtcGetProgramLogSize(rp, &lsz);
      std::string log(lsz, '\0');
      if (lsz) hiprtcGetProgramLog(rp, &log[0]);
      *whyNot = "hiprtc compile failed: " + log;
    }
    hiprtcDestroyProgram(&rp);
    return nullptr;
  }
  size_t csz = 0;
  hiprtcGetCodeSize(rp, &csz);
  std::string code(csz, '\0');
  hiprtcGetCode(rp, &code[0]);
  hiprtcDestroyProgram(&rp);
  hipModule_t mod = nullptr;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess) {
    if (whyNot) *whyNot = "hipModule load failed";
    return nullptr;
  }
  return mod;
}

// compile (cached by source text); returns nullptr on any failure
static const JitProg* compileSource(const std::string& src, const char* fn1,
                                    const char* fn2, std::string* whyNot,
                                    int rowsPerLane = 1) {
  std::lock_guard<std::mutex> lk(cacheMu);
  auto it = cache().find(src);
  if (it != cache().end()) return it->second.ok ? &it->second : nullptr;
  JitProg prog;
  prog.rowsPerLane = rowsPerLane;
  prog.mod = compileModule(src, "genq.cu", whyNot);
  if (prog.mod &&
      hipModuleGetFunction(&prog.fnNarrow, prog.mod, fn1) == hipSuccess &&
      hipModuleGetFunction(&prog.fnWide, prog.mod, fn2) == hipSuccess)
    prog.ok = true;
  else if (prog.mod && whyNot)
    *whyNot = "hipModule load failed";
  auto& slot = cache()[src] = prog;
  return prog.ok ? &slot : nullptr;
}

const JitProg* compile(const FusedQueryDesc& d, bool repl,
                       std::string* whyNot) {
  for (int s = 0; s < d.nAccSlots; s++)
    if (d.accKind[s] == 3) {  // f64 atomics: interpreted kernel only
      if (whyNot) *whyNot = "f64 accumulator not specialized";
      return nullptr;
    }
  for (int a = 0; a < d.nAggs; a++)
    if (d.aggs[a].fcol >= 0) {  // count(f64 column): NULLs read off the bitmap
      if (whyNot) *whyNot = "f64 argument not specialized";
      return nullptr;
    }
  for (int i = 0; i < d.nIns; i++)
    if (d.ins[i].op == gxp::VM_STRLEN) {
      if (whyNot) *whyNot = "string builtin not specialized";
      return nullptr;
    }
  if (!gxp::vmOpsWithin(d.ins, d.nIns, gxp::kVmOpsFull)) {
    // the interpreted kernel raises the flag for such a plan
    if (whyNot) *whyNot = "unknown VM opcode not specialized";
    return nullptr;
  }
  for (int p = 0; p < d.nPreds; p++)
    if (d.preds[p].orWith > 0) {
      if (whyNot) *whyNot = "disjunctive filter not specialized";
      return nullptr;
    }
  if (repl) {
    ReplLayout L;
    if (!planRepl(d, &L)) {
      if (whyNot) *whyNot = "no replicated LDS layout for this plan";
      return nullptr;
    }
  }
  const bool occ8 = wantOcc8(d, repl);
  const int K = rowsPerLane(d);
  const JitProg* prog = compileSource(genSource(d, repl, occ8), "genq_narrow",
                                      "genq_wide", whyNot, K);
  if (prog && occ8) {
    int scratch = 0;
    if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES,
                            prog->fnNarrow) != hipSuccess ||
        scratch > 0)
      prog = compileSource(genSource(d, true, false), "genq_narrow",
                           "genq_wide", whyNot, K);
  }
  return prog;
}

int launch(const JitProg* prog, bool wide, const FusedQueryDesc* devDesc,
           int grid, void* stream) {
  void* args[] = {(void*)&devDesc};
  return (int)hipModuleLaunchKernel(wide ? prog->fnWide : prog->fnNarrow,
                                    grid, 1, 1, 256, 1, 1, 0,
                                    (hipStream_t)stream, args, nullptr);
}


// ---------------------------------------------------------------------
// join-aggregate probe specialization (jaProbeKernel): same idea as the
// fused-agg specialization -- literal fetch/pred/VM/accumulator plans,
// runtime table sizes (slot mask, bloom size) kept as scalar desc reads so
// one compiled kernel serves every step of the executor.
// ---------------------------------------------------------------------
using gxp::JoinAggDesc;

static void emitJaVm(std::ostringstream& s, const JoinAggDesc& d) {
  // registers are never recycled here: max dst + 1 covers every one
  int nRegs = 0;
  for (int i = 0; i < d.nIns; i++)
    if (d.ins[i].dst >= nRegs) nRegs = d.ins[i].dst + 1;
  emitVmRegs(s, nRegs);
  for (int i = 0; i < d.nIns; i++) {
    const gxp::VmIns& ins = d.ins[i];
    std::string v = "v" + std::to_string(ins.dst);
    std::string nv = "n" + std::to_string(ins.dst);
    switch (ins.op) {
      case gxp::VM_LOAD_DEC: {
        const gxp::DevCol& c = d.probe.cols[ins.a];
        s << "  " << v << " = VT<WIDE>::zero(); " << nv << " = false;\n";
        if (c.hasNulls)
          s << "  " << nv << " = colIsNull(d.probe.cols[" << ins.a
            << "], row);\n";
        if (c.units) {
          // proven column: units at the declared frac (= ins.b), read at
          // use at the column's width
          const int w = c.unitsWidth == 1 || c.unitsWidth == 2 ||
                                c.unitsWidth == 4 ? c.unitsWidth : 8;
          s << "  if (!" << nv << ") " << v
            << " = VT<WIDE>::fromI64((int64_t)gptr<int" << 8 * w
            << "_t>(d.probe.cols[" << ins.a << "].units)[row], nullptr);\n";
          break;
        }
        s << "  if (!" << nv << ") { int sc;\n";
        if (ins.c >= 0)
          s << "    if (!parseDecimalRaw<WIDE>(raw.get(" << ins.c << "), &"
            << v << ", &sc, d.errorFlag, " << ins.b << ", " << d.insP10[i]
            << "LL, " << d.insMagic[i] << "ULL)) return false;\n";
        else
          s << "    if (!loadDecimalUnits<WIDE>((const uint8_t*)d.probe.cols["
            << ins.a << "].data + row * 40, &" << v << ", &sc, d.errorFlag, "
            << ins.b << ", " << d.insP10[i] << "LL, " << d.insMagic[i]
            << "ULL)) return false;\n";
        emitDecRescale(s, v, ins.b);
        break;
      }
      case gxp::VM_LOAD_I64: {
        const gxp::DevCol& c = d.probe.cols[ins.a];
        s << "  " << nv << " = false;\n";
        if (c.hasNulls)
          s << "  " << nv << " = colIsNull(d.probe.cols[" << ins.a
            << "], row);\n";
        if (ins.c >= 0)
          s << "  " << v << " = " << nv
            << " ? VT<WIDE>::zero() : VT<WIDE>::fromI64((int64_t)raw.get("
            << ins.c << ").x, &ovf);\n";
        else
          s << "  " << v << " = " << nv
            << " ? VT<WIDE>::zero() : VT<WIDE>::fromI64(gptr<int64_t>(d.probe."
               "cols[" << ins.a << "].data)[row], &ovf);\n";
        break;
      }
      default:
        emitVmOp(s, ins, d.insP10[i], d.constLo, d.constHi);
        break;
    }
  }
}

std::string generateJaSource(const JoinAggDesc& d) {
  std::ostringstream s;
  s << "#include \"gx_common.h\"\n#include \"gx_device.h\"\n"
       "using namespace gxp;\n\n";
  // literal probe-side fetch
  s << "__device__ __forceinline__ void fetchJa(const DevTable& t, int64_t "
       "row, RawState& r) {\n";
  for (int f = 0; f < d.nFetch; f++) {
    const gxp::FetchDesc& fd = d.fetch[f];
    if (fd.kind == gxp::FETCH_B1) continue;
    std::string m = "r.s" + std::to_string(f);
    if (fd.kind == gxp::FETCH_8B)
      s << "  " << m << ".x = gptr<uint64_t>(t.cols[" << fd.col
        << "].data)[row]; " << m << ".y = 0;\n";
    else if (fd.kind == gxp::FETCH_DEC16)
      s << "  { const uint8_t* p = (const uint8_t*)t.cols[" << fd.col
        << "].data + row * 40;\n    " << m << ".x = *gptr<uint64_t>(p); "
        << m << ".y = *gptr<uint64_t>(p + 8); }\n";
  }
  s << "}\n\n";
  s << R"RTC(
__device__ __forceinline__ bool jaBloomMayHave(const JoinAggDesc& d, uint64_t key) {
  if (d.bloomLog2 == 0) return true;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloomLog2) - 1;
  uint32_t b1 = (uint32_t)h & mask;
  uint32_t b2 = (uint32_t)(h >> 32) & mask;
  auto bm = gptr<uint32_t>(d.bloom);
  if (!((bm[b1 >> 5] >> (b1 & 31)) & 1)) return false;
  return ((bm[b2 >> 5] >> (b2 & 31)) & 1) != 0;
}

template <bool WIDE>
__device__ __forceinline__ bool jaRow(const JoinAggDesc& d, int64_t row,
                                      uint32_t mask, uint64_t* myMatch) {
  using T = typename VT<WIDE>::T;
  bool ovf = false; (void)ovf;
  RawState raw;
  fetchJa(d.probe, row, raw);
)RTC";
  // literal predicate
  if (d.nPredP > 0) {
    const gxp::PredDesc& pd = d.predP;
    const gxp::DevCol& c = d.probe.cols[pd.col];
    if (c.hasNulls)
      s << "  if (colIsNull(d.probe.cols[" << pd.col
        << "], row)) return true;\n";
    if (pd.kind == gxp::PRED_TIME_CMP_CONST) {
      s << "  { uint64_t pv = "
        << (pd.slot >= 0
                ? ("raw.get(" + std::to_string(pd.slot) + ").x")
                : ("gptr<uint64_t>(d.probe.cols[" + std::to_string(pd.col) +
                   "].data)[row]"))
        << " & ~0xFULL;\n    if (!(pv " << cmpOp(pd.cmp) << " "
        << (pd.constU64 & ~0xFULL) << "ULL)) return true; }\n";
    } else if (pd.kind == gxp::PRED_I64_CMP_CONST) {
      s << "  { int64_t pv = "
        << (pd.slot >= 0
                ? ("(int64_t)raw.get(" + std::to_string(pd.slot) + ").x")
                : ("gptr<int64_t>(d.probe.cols[" + std::to_string(pd.col) +
                   "].data)[row]"))
        << ";\n    if (!(pv " << cmpOp(pd.cmp) << " (int64_t)"
        << (int64_t)pd.constU64 << "LL)) return true; }\n";
    } else if (pd.kind == gxp::PRED_STR_LIKE) {
      // general LIKE: shared matcher, pattern inside the PredDesc
      s << "  if (!evalSimplePred(d.probe, d.predP, d.strConst, "
           "d.strConstLen, row)) return true;\n";
    }
  }
  // key + bloom + slot probe
  const gxp::DevCol& kc = d.probe.cols[d.pKeyCol];
  if (kc.hasNulls)
    s << "  if (colIsNull(d.probe.cols[" << d.pKeyCol
      << "], row)) return true;\n";
  s << "  uint64_t key = gptr<uint64_t>(d.probe.cols[" << d.pKeyCol
    << "].data)[row];\n"
       "  if (key == kEmptyKey) key = kEmptyKey - 1;\n"
       "  if (!jaBloomMayHave(d, key)) return true;\n"
       "  uint32_t slot = (uint32_t)(splitmix64(key) & mask);\n"
       "  bool found = false;\n"
       "  for (uint32_t probe = 0; probe <= mask; probe++) {\n"
       "    uint64_t cur = gptr<uint64_t>(&d.slots[slot].key)[0];\n"
       "    if (cur == key) { found = true; break; }\n"
       "    if (cur == kEmptyKey) break;\n"
       "    slot = (slot + 1) & mask;\n"
       "  }\n"
       "  if (!found) return true;\n"
       "  {\n";
  emitJaVm(s, d);
  s << "    if (ovf) { atomicOr(d.errorFlag, WIDE ? kErrOverflow : "
       "kErrRetryWide); return false; }\n";
  s << "    if (n" << d.valueReg << ") return true;\n"
    << "    Int128 vv = VT<WIDE>::toAcc(v" << d.valueReg << ");\n";
  s << R"RTC(
    JoinAggSlot* sp = &d.slots[slot];
    uint64_t old = atomicAdd((unsigned long long*)&sp->accLo, (unsigned long long)vv.lo);
    uint64_t carry = (old + vv.lo) < old ? 1 : 0;
    int64_t hiAdd = vv.hi + (int64_t)carry;
    if (hiAdd != 0)
      atomicAdd((unsigned long long*)&sp->accHi, (unsigned long long)hiAdd);
    if (vv.hi < 0 || (vv.hi == 0 && vv.lo == 0))
      atomicAdd((unsigned long long*)&sp->cnt, 1ULL);
    (*myMatch)++;
  }
  return true;
}

template <bool WIDE>
__device__ __forceinline__ void jaBody(const JoinAggDesc* __restrict__ dp) {
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
    if (!jaRow<WIDE>(d, row, mask, &myMatch)) failed = true;
  }
  for (int off = 32; off > 0; off >>= 1) myMatch += __shfl_down(myMatch, off, 64);
  if ((threadIdx.x & 63) == 0 && myMatch)
    atomicAdd((unsigned long long*)&d.counters[2], (unsigned long long)myMatch);
}

extern "C" __global__ void __launch_bounds__(256) genja_narrow(const JoinAggDesc* __restrict__ dp) {
  jaBody<false>(dp);
}
extern "C" __global__ void __launch_bounds__(256) genja_wide(const JoinAggDesc* __restrict__ dp) {
  jaBody<true>(dp);
}
)RTC";
  return s.str();
}

const JitProg* compileJa(const JoinAggDesc& d, std::string* whyNot) {
  if (d.nPredP > 0 && d.predP.kind != gxp::PRED_TIME_CMP_CONST &&
      d.predP.kind != gxp::PRED_I64_CMP_CONST) {
    if (whyNot) *whyNot = "probe predicate kind not specialized";
    return nullptr;
  }
  if (d.chained || d.nPredPx > 0) {
    if (whyNot) *whyNot = "chained/multi-conjunct probe not specialized";
    return nullptr;
  }
  if (!gxp::vmOpsWithin(d.ins, d.nIns, gxp::kVmOpsCore)) {
    // the interpreted probe kernel raises the flag for such a plan
    if (whyNot) *whyNot = "VM opcode outside the probe set not specialized";
    return nullptr;
  }
  std::string src = generateJaSource(d);
  return compileSource(src, "genja_narrow", "genja_wide", whyNot);
}


int launchJa(const JitProg* prog, bool wide, const JoinAggDesc* devDesc,
             int grid, void* stream) {
  void* args[] = {(void*)&devDesc};
  return (int)hipModuleLaunchKernel(wide ? prog->fnWide : prog->fnNarrow,
                                    grid, 1, 1, 256, 1, 1, 0,
                                    (hipStream_t)stream, args, nullptr);
}

// build-phase specialization: four straight-line kernels (count0, build0,
// count1, build1). count1/build1 scan the big middle table (orders at Q3):
// their per-row chain is two dependent 8B loads + a key-set probe, so the
// emitted loop software-pipelines the predicate-column load one stride
// ahead (the interpreted versions measured latency-bound at ~5x their
// sequential-traffic floor).
static void emitPredInline(std::ostringstream& s, const JoinAggDesc& d,
                           const gxp::PredDesc& pd, const char* tbl,
                           const char* rowVar, const char* preVar) {
  const gxp::DevCol& c =
      (std::string(tbl) == "d.build0" ? d.build0 : d.build1).cols[pd.col];
  if (c.hasNulls)
    s << "    if (colIsNull(" << tbl << ".cols[" << pd.col << "], " << rowVar
      << ")) continue;\n";
  if (pd.kind == gxp::PRED_TIME_CMP_CONST) {
    s << "    { uint64_t pv = " << (preVar ? preVar : "0");
    if (!preVar)
      s << "; pv = gptr<uint64_t>(" << tbl << ".cols[" << pd.col << "].data)["
        << rowVar << "]";
    s << "; pv &= ~0xFULL;\n      if (!(pv " << cmpOp(pd.cmp) << " "
      << (pd.constU64 & ~0xFULL) << "ULL)) continue; }\n";
  } else if (pd.kind == gxp::PRED_I64_CMP_CONST) {
    s << "    { int64_t pv = (int64_t)" << (preVar ? preVar : "0");
    if (!preVar)
      s << "; pv = gptr<int64_t>(" << tbl << ".cols[" << pd.col << "].data)["
        << rowVar << "]";
    s << ";\n      if (!(pv " << cmpOp(pd.cmp) << " (int64_t)"
      << (int64_t)pd.constU64 << "LL)) continue; }\n";
  } else if (pd.kind == gxp::PRED_STR_LIKE) {
    // general LIKE: shared matcher, pattern inside the PredDesc
    const char* pdName = &pd == &d.pred0 ? "d.pred0" : "d.pred1";
    s << "    if (!evalSimplePred(" << tbl << ", " << pdName
      << ", d.strConst, d.strConstLen, " << rowVar << ")) continue;\n";
  } else {  // PRED_STR_EQ_CONST: literal bytes
    s << "    { int64_t st, en;\n";
    if (c.denseOffsets)
      s << "      st = " << rowVar << "; en = " << rowVar << " + 1;\n";
    else
      s << "      st = gptr<int64_t>(" << tbl << ".cols[" << pd.col
        << "].offsets)[" << rowVar << "]; en = gptr<int64_t>(" << tbl
        << ".cols[" << pd.col << "].offsets)[" << rowVar << " + 1];\n";
    s << "      auto p = gptr<uint8_t>(" << tbl << ".cols[" << pd.col
      << "].data);\n"
         "      while (en > st && p[en - 1] == ' ') en--;\n"
         "      if (en - st != " << d.strConstLen << ") continue;\n"
         "      bool eq = true;\n";
    for (int b = 0; b < d.strConstLen; b++)
      s << "      eq = eq && p[st + " << b << "] == " << (int)d.strConst[b]
        << ";\n";
    s << "      if (" << (pd.cmp == 4 ? "!eq" : "eq") << ") continue; }\n";
  }
}

std::string generateJaBuildSource(const JoinAggDesc& d) {
  std::ostringstream s;
  s << "#include \"gx_common.h\"\n#include \"gx_device.h\"\nusing namespace "
       "gxp;\n\n";
  s << R"RTC(
__device__ __forceinline__ bool jaKeySetHas(const JoinAggDesc& d, uint64_t key) {
  uint32_t mask = (1u << d.keySetLog2) - 1;
  if (key == kEmptyKey) key = kEmptyKey - 1;
  uint32_t slot = (uint32_t)(splitmix64(key) & mask);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    uint64_t cur = gptr<uint64_t>(d.keySet)[slot];
    if (cur == key) return true;
    if (cur == kEmptyKey) return false;
    slot = (slot + 1) & mask;
  }
  return false;
}
__device__ __forceinline__ bool jaBloom0MayHave(const JoinAggDesc& d, uint64_t key) {
  if (d.bloom0Log2 == 0) return true;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloom0Log2) - 1;
  uint32_t b1 = (uint32_t)h & mask;
  uint32_t b2 = (uint32_t)(h >> 32) & mask;
  auto bm = gptr<uint32_t>(d.bloom0);
  if (!((bm[b1 >> 5] >> (b1 & 31)) & 1)) return false;
  return ((bm[b2 >> 5] >> (b2 & 31)) & 1) != 0;
}
__device__ __forceinline__ void jaBloom0Set(const JoinAggDesc& d, uint64_t key) {
  if (d.bloom0Log2 == 0) return;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloom0Log2) - 1;
  atomicOr(&d.bloom0[((uint32_t)h & mask) >> 5], 1u << ((uint32_t)h & 31));
  atomicOr(&d.bloom0[((uint32_t)(h >> 32) & mask) >> 5],
           1u << ((uint32_t)(h >> 32) & 31));
}
__device__ __forceinline__ void jaBloomSet(const JoinAggDesc& d, uint64_t key) {
  if (d.bloomLog2 == 0) return;
  uint64_t h = splitmix64(key);
  uint32_t mask = (1u << d.bloomLog2) - 1;
  atomicOr(&d.bloom[((uint32_t)h & mask) >> 5], 1u << ((uint32_t)h & 31));
  atomicOr(&d.bloom[((uint32_t)(h >> 32) & mask) >> 5],
           1u << ((uint32_t)(h >> 32) & 31));
}
)RTC";
  // ---- count0 / build0 over build0 (customer) ----
  s << R"RTC(
extern "C" __global__ void __launch_bounds__(256) genja_count0(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build0.nRows;
  uint64_t my = 0;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
)RTC";
  if (d.nPred0 > 0) emitPredInline(s, d, d.pred0, "d.build0", "row", nullptr);
  if (d.build0.cols[d.b0KeyCol].hasNulls)
    s << "    if (colIsNull(d.build0.cols[" << d.b0KeyCol
      << "], row)) continue;\n";
  s << R"RTC(    my++;
  }
  for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, off, 64);
  if ((threadIdx.x & 63) == 0 && my)
    atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)my);
}

extern "C" __global__ void __launch_bounds__(256) genja_build0(const JoinAggDesc* __restrict__ dp) {
  const JoinAggDesc& d = *dp;
  int64_t n = d.build0.nRows;
  uint32_t mask = (1u << d.keySetLog2) - 1;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n;
       row += (int64_t)gridDim.x * blockDim.x) {
)RTC";
  if (d.nPred0 > 0) emitPredInline(s, d, d.pred0, "d.build0", "row", nullptr);
  if (d.build0.cols[d.b0KeyCol].hasNulls)
    s << "    if (colIsNull(d.build0.cols[" << d.b0KeyCol
      << "], row)) continue;\n";
  s << "    uint64_t key = gptr<uint64_t>(d.build0.cols[" << d.b0KeyCol
    << "].data)[row];\n";
  s << R"RTC(    if (key == kEmptyKey) key = kEmptyKey - 1;
    jaBloom0Set(d, key);
    uint32_t slot = (uint32_t)(splitmix64(key) & mask);
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
)RTC";
  // ---- count1 / build1 over build1 (orders): 2-deep pipelined pred load ---
  // (only when the predicate is a slotless 8B compare; else plain loop)
  bool pipe1 = d.nPred1 > 0 && (d.pred1.kind == gxp::PRED_TIME_CMP_CONST ||
                                d.pred1.kind == gxp::PRED_I64_CMP_CONST) &&
               !d.build1.cols[d.pred1.col].hasNulls;
  auto emitB1Loop = [&](bool counting) {
    const char* fn = counting ? "genja_count1" : "genja_build1";
    s << "extern \"C\" __global__ void __launch_bounds__(256) " << fn
      << "(const JoinAggDesc* __restrict__ dp) {\n"
         "  const JoinAggDesc& d = *dp;\n"
         "  int64_t n = d.build1.nRows;\n";
    if (!counting) s << "  uint32_t mask = (1u << d.slotsLog2) - 1;\n";
    if (counting) s << "  uint64_t my = 0;\n";
    s << "  const int64_t stride = (int64_t)gridDim.x * blockDim.x;\n"
         "  int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;\n";
    if (pipe1) {
      s << "  uint64_t preA = row < n ? gptr<uint64_t>(d.build1.cols["
        << d.pred1.col << "].data)[row] : 0;\n";
    }
    s << "  for (; row < n; row += stride) {\n";
    if (pipe1) {
      s << "    uint64_t preCur = preA;\n"
           "    { int64_t rn = row + stride;\n"
           "      if (rn < n) preA = gptr<uint64_t>(d.build1.cols["
        << d.pred1.col << "].data)[rn]; }\n";
      emitPredInline(s, d, d.pred1, "d.build1", "row", "preCur");
    } else if (d.nPred1 > 0) {
      emitPredInline(s, d, d.pred1, "d.build1", "row", nullptr);
    }
    if (d.build1.cols[d.b1ProbeCol].hasNulls)
      s << "    if (colIsNull(d.build1.cols[" << d.b1ProbeCol
        << "], row)) continue;\n";
    s << "    uint64_t pkey0 = gptr<uint64_t>(d.build1.cols[" << d.b1ProbeCol
      << "].data)[row];\n"
         "    if (!jaBloom0MayHave(d, pkey0)) continue;\n"
         "    if (!jaKeySetHas(d, pkey0)) continue;\n";
    if (counting) {
      s << "    my++;\n  }\n"
           "  for (int off = 32; off > 0; off >>= 1) my += __shfl_down(my, "
           "off, 64);\n"
           "  if ((threadIdx.x & 63) == 0 && my)\n"
           "    atomicAdd((unsigned long long*)&d.counters[1], (unsigned long "
           "long)my);\n}\n\n";
      return;
    }
    if (d.build1.cols[d.b1KeyCol].hasNulls)
      s << "    if (colIsNull(d.build1.cols[" << d.b1KeyCol
        << "], row)) continue;\n";
    s << "    uint64_t key = gptr<uint64_t>(d.build1.cols[" << d.b1KeyCol
      << "].data)[row];\n"
         "    if (key == kEmptyKey) key = kEmptyKey - 1;\n";
    if (d.payloadCol0 >= 0)
      s << "    uint64_t pay0 = gptr<uint64_t>(d.build1.cols[" << d.payloadCol0
        << "].data)[row];\n";
    else
      s << "    uint64_t pay0 = 0;\n";
    if (d.payloadCol1 >= 0)
      s << "    int64_t pay1 = gptr<int64_t>(d.build1.cols[" << d.payloadCol1
        << "].data)[row];\n";
    else
      s << "    int64_t pay1 = 0;\n";
    s << R"RTC(    jaBloomSet(d, key);
    uint32_t slot = (uint32_t)(splitmix64(key) & mask);
    for (uint32_t probe = 0; probe <= mask; probe++) {
      uint64_t cur = d.slots[slot].key;
      if (cur == key) { atomicOr(d.errorFlag, kErrBadKey); break; }
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

)RTC";
  };
  emitB1Loop(true);
  emitB1Loop(false);
  return s.str();
}

struct JaBuildProg {
  hipModule_t mod = nullptr;
  hipFunction_t fn[4] = {nullptr, nullptr, nullptr, nullptr};  // c0,b0,c1,b1
  bool ok = false;
};

static std::map<std::string, JaBuildProg>& buildCache() {
  static std::map<std::string, JaBuildProg> c;
  return c;
}

const JaBuildProg* compileJaBuild(const JoinAggDesc& d, std::string* whyNot) {
  if (d.chained || d.nPred0x > 0 || d.nPred1x > 0) {
    if (whyNot) *whyNot = "chained/multi-conjunct build not specialized";
    return nullptr;
  }
  std::string src = generateJaBuildSource(d);
  std::lock_guard<std::mutex> lk(cacheMu);
  auto it = buildCache().find(src);
  if (it != buildCache().end()) return it->second.ok ? &it->second : nullptr;
  JaBuildProg prog;
  prog.mod = compileModule(src, "genjab.cu", whyNot);
  if (!prog.mod) {
    buildCache()[src] = prog;
    return nullptr;
  }
  static const char* names[4] = {"genja_count0", "genja_build0",
                                 "genja_count1", "genja_build1"};
  bool ok = true;
  for (int i = 0; ok && i < 4; i++)
    ok = hipModuleGetFunction(&prog.fn[i], prog.mod, names[i]) == hipSuccess;
  if (!ok) {
    if (whyNot) *whyNot = "hipModule load failed";
    buildCache()[src] = prog;
    return nullptr;
  }
  prog.ok = true;
  auto& slot = buildCache()[src] = prog;
  return &slot;
}

int launchJaBuild(const JaBuildProg* prog, int phase,
                  const JoinAggDesc* devDesc, int grid, void* stream) {
  void* args[] = {(void*)&devDesc};
  return (int)hipModuleLaunchKernel(prog->fn[phase], grid, 1, 1, 256, 1, 1, 0,
                                    (hipStream_t)stream, args, nullptr);
}

}  // namespace gxjit
