// tidb_amd/csrc/gx_engine.cpp — MI355X product engine: C-ABI implementation.
//
// Drop-in for the reference executor tree behind exec.Executor
// (pkg/executor/internal/exec/executor.go:224-250): the engine compiles the
// plan (Source -> [Selection] -> [Projection] -> HashAgg) into ONE fused HIP
// kernel pass (gx_kernels.hip) — columns resident in HBM, chunks cross
// host<->device only at the tree fringe (source bind, final small results).
//
// There is NO CPU fallback for the compute path: a plan that needs the GPU
// fails loudly (GX_ERR_NO_GPU) when no MI355X is reachable. The only host
// compute is the O(#groups) finalize (avg DecimalDiv + Round — the reference
// does this once per group too, func_avg.go:84-109) and the FINAL-mode merge
// of canonical partial states (KB-sized; MergePartialResult semantics,
// aggfuncs.go:250-255).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <functional>
#include <set>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gx_executor.h"
#include "gx_common.h"
#include "gx_decimal.h"
#include "gx_jit.h"
#include "gx_result.h"

using gxp::HostCol;
using gxp::MyDecimal;
using gxp::OutRowVal;
using gxp::ResultRow;
using gxp::decFromUnits;

namespace {

// ---------------- plan IR (mirrors the C-ABI builder calls) ----------------
enum { EK_COLREF, EK_CONST, EK_CALL };
enum { PK_SOURCE, PK_SELECTION, PK_PROJECTION, PK_HASHAGG, PK_TOPN, PK_HASHJOIN,
       PK_STREAMAGG, PK_MERGEJOIN };

struct PExpr {
  int kind = EK_COLREF;
  int retType = GX_TYPE_I64;
  int retFrac = 0;
  int colIdx = -1;
  int func = -1;
  std::vector<int> args;
  int64_t constI64 = 0;
  double constF64 = 0;
  uint64_t constTime = 0;
  MyDecimal constDec;
  std::string constStr;
};

struct PNode {
  int kind = PK_SOURCE;
  int child = -1, child2 = -1;
  std::vector<int> colTypes, colFracs;
  std::vector<int> exprs;
  std::vector<int> aggFuncs, aggArgs, aggFracs;
  int aggMode = 0;
  std::vector<uint8_t> keyDesc;
  int64_t limit = 0, offset = 0;
  std::vector<int> buildKeys, probeKeys;
  int joinType = 0;
};

struct PPlan {
  std::vector<PExpr> exprs;
  std::vector<PNode> nodes;
};

struct Binding {
  bool haveChunks = false;
  std::vector<std::vector<HostCol>> chunks;
  int tpchTable = -1;
  int64_t tpchRows = 0, tpchRowOffset = 0, tpchTotalRows = 0;
  uint64_t tpchSeed = 42;
};

// one host-resident sorted run of the out-of-core sort (the spill container
// analog of sortexec/sort_spill.go + chunk.DataInDiskByChunks — host RAM
// stands in for disk; runs stream back through the k-way merge on emission,
// multi_way_merge.go semantics)
struct SortRun {
  std::vector<std::vector<uint8_t>> colData;   // per col: n x elem bytes
  std::vector<std::vector<uint64_t>> keys;     // per sort key: composed
                                               // order-preserving u64 per row
  int64_t n = 0;
};

// one host-resident hash partition of an out-of-core join side — the
// partition-file analog of join/hash_join_spill.go (host RAM stands in for
// disk, like the sort-spill runs). Rows of one join key land in exactly one
// partition on both sides, so the partitions join independently.
struct JoinPart {
  std::vector<std::vector<uint8_t>> colData;     // per col: bytes
  std::vector<std::vector<int64_t>> colOffsets;  // varlen: n+1 (else empty)
  std::vector<std::vector<uint8_t>> nullBytes;   // byte/row (else empty)
  int64_t n = 0;
};

}  // namespace

struct gx_exec;

// ---- host expression compiler: one for the fused, probe and projection
// VMs ----
// Projection's kernel runs the full step, but its host site has never lowered
// division; enabling it there is a separate change.
constexpr uint32_t kVmOpsProject = gxp::kVmOpsFull & ~(1u << gxp::VM_DIV);
// the probe and projection kernels hold a 12-register VmState
constexpr int kVmRegsNarrowState = 12;

// Lowers PExpr trees to VmIns for one site (vmCompile). The site binds its
// descriptor's program fields, the schema the expressions run over, the
// opcode set its kernel executes and its register budget. Fetch slots are
// never assigned here: loads carry c = -1.
struct ExprBuilder {
  // target program (the three descriptors share these field names)
  gxp::VmIns* ins = nullptr;
  int32_t* nIns = nullptr;
  int64_t* constLo = nullptr;
  int64_t* constHi = nullptr;
  int32_t* nConsts = nullptr;
  int64_t* insP10 = nullptr;
  uint64_t* insMagic = nullptr;
  int32_t* wide = nullptr;
  gxp::LikePat* likePats = nullptr;  // VM_LIKE pattern table, if the site has one
  int32_t* nLikePats = nullptr;
  // schema the program runs over; colBase = plan colref index of its column 0
  const std::vector<int>* colTypes = nullptr;
  const std::vector<int>* colFracs = nullptr;
  int colBase = 0;
  uint32_t ops = 0;  // opcode set of the site's kernel (gxp::kVmOps*)
  // registers: bump allocation up to maxRegs. With consumer counts
  // (countConsumers) a derived value's register returns to the free list
  // after its last consumer is emitted, so wide projections fit.
  int maxRegs = 0;
  int nextReg = 0;
  bool recycle = false;
  std::map<int, int> exprUse;  // remaining consumers per expression
  std::vector<int> freeRegs;
  std::map<int, std::pair<int, int>> memo;  // exprId -> (reg, scale)
  bool hasDiv = false;  // DIV forces the wide VM and disables glds

  template <class Desc>
  void bind(Desc& d, const std::vector<int>* types,
            const std::vector<int>* fracs, int base, uint32_t opSet, int regs) {
    ins = d.ins;
    nIns = &d.nIns;
    constLo = d.constLo;
    constHi = d.constHi;
    nConsts = &d.nConsts;
    insP10 = d.insP10;
    insMagic = d.insMagic;
    wide = &d.wide;
    colTypes = types;
    colFracs = fracs;
    colBase = base;
    ops = opSet;
    maxRegs = regs;
  }
  template <class Desc>
  void bindLikePats(Desc& d) {
    likePats = d.likePats;
    nLikePats = &d.nLikePats;
  }

  // Consumer counts over the expression DAG below `roots`; supplying them
  // turns recycling on. Roots are pinned outputs: never counted, never
  // released (a root may also appear as a subexpression, e.g. a projected
  // value the cast of which is also projected).
  void countConsumers(const PPlan& plan, const std::vector<int>& roots) {
    std::set<int> visited;
    std::function<void(int)> cnt = [&](int id) {
      for (int a : plan.exprs[id].args) {
        exprUse[a]++;
        if (visited.insert(a).second) cnt(a);
      }
    };
    for (int r : roots) cnt(r);
    for (int r : roots) exprUse.erase(r);
    recycle = true;
  }

  int allocReg() {
    if (recycle && !freeRegs.empty()) {
      int r = freeRegs.back();
      freeRegs.pop_back();
      return r;
    }
    return allocRegFresh();
  }
  // Loads are MOVED to the front of the instruction stream (the grouped
  // fetch pipeline); a load's destination register must therefore never be
  // a recycled one -- an instruction that originally preceded the load and
  // wrote that register would execute after it post-reorder and clobber the
  // loaded value. Fresh registers only for loads.
  int allocRegFresh() {
    if (nextReg >= maxRegs) {
      if (getenv("GX_DEBUG"))
        fprintf(stderr, "[gx] reg exhausted (nIns=%d, memo=%d)\n", *nIns,
                (int)memo.size());
      return -1;
    }
    return nextReg++;
  }
  // an anonymous scale-up temporary dies with the op that consumed it
  void freeTemp(int reg) {
    if (recycle && reg >= 0) freeRegs.push_back(reg);
  }
  // emitted the last consumer of argExpr -> recycle its register
  void release(int argExpr) {
    if (!recycle) return;
    auto u = exprUse.find(argExpr);
    if (u == exprUse.end()) return;  // pinned (projection root) or unknown
    if (--u->second > 0) return;
    auto c = memo.find(argExpr);
    if (c == memo.end()) return;
    // aliased entries (no-op casts) share a register: keep it live while
    // any other expression still maps to it
    for (auto& kv : memo)
      if (kv.first != argExpr && kv.second.first == c->second.first) return;
    // LOAD results must stay cached: the loads-first reorder hands their
    // slots to the fetch pipeline once; recompiling one later would add a
    // second load of the same column. Only recycle derived values.
    int op = -1;
    for (int i = 0; i < *nIns; i++)
      if (ins[i].dst == c->second.first) op = ins[i].op;
    if (op == gxp::VM_LOAD_DEC || op == gxp::VM_LOAD_I64 ||
        op == gxp::VM_LOAD_CONST)
      return;
    freeRegs.push_back(c->second.first);
    memo.erase(c);
  }

  // Screens `op` against the site's set: an opcode the site's kernel does
  // not run is a plan error here, not a device error at run time.
  bool allowed(gx_exec* ex, int op) const;
  int emit(gx_exec* ex, int op, int dst, int a, int b, int c = -1) {
    if (!allowed(ex, op)) return -1;
    if (dst < 0 || *nIns >= gxp::kMaxVmIns) return -1;
    ins[(*nIns)++] = {op, dst, a, b, c};
    return dst;
  }
  // ra, rb at scales sa, sb -> both at max(sa, sb), the result frac of
  // MySQL add/sub/compare/IF; tmpA/tmpB receive the scale-up temporaries
  int alignScales(gx_exec* ex, int* ra, int sa, int* rb, int sb, int* tmpA,
                  int* tmpB) {
    int target = std::max(sa, sb);
    *tmpA = *tmpB = -1;
    if (sa < target)
      *tmpA = *ra = emit(ex, gxp::VM_SCALE_UP, allocReg(), *ra, target - sa);
    if (sb < target)
      *tmpB = *rb = emit(ex, gxp::VM_SCALE_UP, allocReg(), *rb, target - sb);
    return target;
  }
};

struct gx_pb {
  PPlan plan;
};

// How an executor runs its plan. FUSED: fused aggregation over one source.
// AGG_OVER_JOIN: join stages materialize the joined rows, the fused
// aggregation runs over that table. FINAL_HOST: FINAL-mode merge of partial
// chunks on the host. BARE_SOURCE: a bound source, optionally device-sorted.
// JOIN_AGG: the Q3-class join-aggregate pipeline. HASH_JOIN, SELECT, PROJECT:
// the standalone operators, materialized as a device table.
enum class ExecKind {
  NONE, FUSED, AGG_OVER_JOIN, FINAL_HOST, BARE_SOURCE, JOIN_AGG, HASH_JOIN,
  SELECT, PROJECT
};

struct gx_exec {
  PPlan plan;
  int root = -1;
  int device = -1;
  std::map<int, Binding> bindings;
  std::string err;
  bool opened = false;

  // the route that took the plan: set once, by gx_build's router, after the
  // route's compiler succeeds (NONE = not executable)
  ExecKind kind = ExecKind::NONE;
  // FUSED and AGG_OVER_JOIN run the fused aggregation kernel over desc
  bool usesFusedDesc() const {
    return kind == ExecKind::FUSED || kind == ExecKind::AGG_OVER_JOIN;
  }
  // the join-aggregate compile met a value-context LIKE: a plan error, not a
  // reason to fall back to aggregation over materialized joined rows
  bool jaLikeRejected = false;
  // compiled fused query
  int aggRoot = -1;  // the HASHAGG node the fused kernel implements
  // DISTINCT rewrite (aggFuncDesc.HasDistinct): the device kernel groups by
  // (orig keys..., arg) — the dedup — and the decode folds back to the orig
  // keys. distinct.nKeys >= 0 marks the rewrite; funcs/fracs are the USER's;
  // argSlot holds appended-key indices (tuple args have several).
  gxp::DistinctSpec distinct;
  // HAVING: Selection over the agg output, compiled at build
  // (compileHaving), filtered on host over the decoded group rows
  std::vector<gxp::HavingCond> having;
  int sourceNode = -1;
  gxp::FusedQueryDesc desc;
  std::vector<std::pair<int, int>> projRegs;  // projection idx -> (reg, scale)
  ExprBuilder vm;  // fused expression compile state (reset by compileFused)
  // hipRTC-specialized kernel for this plan (gx_jit.cpp); nullptr -> use the
  // interpreted fusedAggKernel
  const gxjit::JitProg* jitProg = nullptr;
  bool jitTried = false;
  // the same plan with lane-replicated LDS accumulators (accumulation tier
  // 0); ldsNoRepl = a block outgrew its small key table, sticky like noLds
  const gxjit::JitProg* jitProgRepl = nullptr;
  bool jitReplTried = false;
  bool ldsNoRepl = false;
  int lastLdsTier = -1;  // tier of the last fused pass (gx_debug_lds_tier)
  const gxjit::JitProg* jaJitProg = nullptr;
  bool jaJitTried = false;
  const gxjit::JaBuildProg* jaBuildProg = nullptr;
  bool jaBuildTried = false;
  // device state
  bool deviceReady = false;
  bool fusedStreamed = false;  // out-of-core agg ran (re-opens re-stream)
  std::vector<void*> devBufs;
  // persistent singletons (descriptors, counters, result tables) whose
  // pointers are cached across runs — never freed by beginRun/freeSince
  std::vector<void*> persistBufs;
  // index into devBufs where the current run's allocations begin (SIZE_MAX
  // until the first run); see beginRun()
  size_t runMark = SIZE_MAX;
  gxp::GroupSlot* devTable = nullptr;
  gxp::FusedQueryDesc* devDesc = nullptr;
  uint32_t* devErr = nullptr;
  uint64_t* devSel = nullptr;
  // fused pass result block (devErr/devSel point into its header) and the
  // pinned host copy one hipMemcpyAsync per open lands in; resultCompact =
  // the last pass ran compactGroupsKernel, so hostResult holds the groups
  gxp::FusedResultBlock* devResult = nullptr;
  gxp::FusedResultBlock* hostResult = nullptr;
  bool resultCompact = false;
  bool lastDecodeCompact = false;  // gx_debug_result_compact
  // kernel-time events, created once per executor
  hipEvent_t evK0 = nullptr, evK1 = nullptr;
  // host shadow of the descriptor as last uploaded to devDesc
  std::vector<uint8_t> descShadow;
  hipStream_t stream = nullptr;
  // results
  bool ranQuery = false;
  std::vector<ResultRow> resultRows;
  size_t emitPos = 0;
  // bare-source emit state
  int64_t srcPos = 0;
  int64_t sliceStart = 0;  // first row of the OFFSET/LIMIT slice, for re-open
  // device full sort over a bare source (sortexec/sort.go analog)
  std::vector<gxp::SortKeyCompose> devSortKeys;
  bool devSorted = false;
  int64_t devSortLimit = -1, devSortOffset = 0;
  // out-of-core sort: device-sorted runs spilled to host, k-way merged on
  // emission (triggered when the table exceeds the HBM budget or
  // GX_SORT_RUN_ROWS forces a run size)
  bool spillSorted = false;
  std::vector<SortRun> sortRuns;
  std::vector<int64_t> runPos;
  int64_t spillSkip = 0;        // offset countdown
  int64_t spillRemaining = -1;  // limit countdown (-1 = unlimited)
  uint64_t lastSelCount = 0;
  double lastKernelMs = 0;
  // GX_DEBUG host-side split of one fused open: microseconds per segment
  // (upload, launch, sync + result block copy, full-table download when the
  // compact block does not answer, decode)
  struct HostSplit {
    bool on = false;
    std::chrono::steady_clock::time_point last;
    double us[7] = {0, 0, 0, 0, 0, 0, 0};
    void begin() {
      on = getenv("GX_DEBUG") != nullptr;
      if (!on) return;
      for (double& u : us) u = 0;
      last = std::chrono::steady_clock::now();
    }
    void lap(int seg) {
      if (!on) return;
      auto now = std::chrono::steady_clock::now();
      us[seg] += std::chrono::duration<double, std::micro>(now - last).count();
      last = now;
    }
    void print() const {
      if (!on) return;
      fprintf(stderr,
              "[gx] host split us: upload=%.1f launch=%.1f sync+d2h=%.1f "
              "d2h_table=%.1f decode=%.1f\n",
              us[0], us[1], us[2], us[5], us[6]);
    }
  } split;

  // post-aggregation host sort (ORDER BY / TopN over the fused agg output)
  bool postSort = false;
  std::vector<std::pair<int, bool>> postSortKeys;  // (agg output col, desc)
  int64_t postLimit = -1, postOffset = 0;

  // join-agg (Q3-class) state
  gxp::JoinAggDesc ja;
  int jaSrcCust = -1, jaSrcOrd = -1, jaSrcLi = -1;
  gxp::JoinAggDesc* devJa = nullptr;
  int jaValueScale = 0;
  int jaAggFrac = 0;  // the SUM's declared result frac
  // output mapping: for each group column: 0 = probe key, 1 = payload0,
  // 2 = payload1; types of the payload cols
  std::vector<int> jaGroupSrc;
  std::vector<int> jaGroupType;
  // topn keys: (column index into the agg output row, desc?)
  std::vector<std::pair<int, bool>> jaSortKeys;
  int64_t jaLimit = 0, jaOffset = 0;

  // standalone hash join (inner, duplicate build keys) state.
  // A join subtree compiles into a topologically ordered list of STAGES
  // (nested joins materialize bottom-up: a stage's side is either a bound
  // source or a previous stage's materialized output table).
  struct JoinStage {
    gxp::HashJoinDesc hj;
    int srcB = -1, srcP = -1;            // source plan-node ids, or -1
    int buildStage = -1, probeStage = -1;  // feeding stage index, or -1
    std::vector<int> types, fracs;       // output schema (build ++ probe)
    gxp::DevTable out;                   // materialized output (run time)
    bool inputsReady = false;            // sources materialized once
    gxp::DevTable buildTab, probeTab;    // resident side tables
  };
  std::vector<JoinStage> joinStages;     // root stage last
  // out-of-core join (hash_join_spill.go analog): both sides hash-partition
  // into host-RAM runs when build+probe+output exceed the HBM budget;
  // partitions join one at a time on device, streaming out per partition
  bool joinSpill = false;
  int joinSpillCur = -1;
  size_t joinSpillMark = SIZE_MAX;
  std::vector<JoinPart> spillB, spillP;
  // null-aware joins (types 5, 7) under spill: passing build rows and NULL
  // build keys of the WHOLE build side, summed while partitioning it
  uint64_t spillBuildPass = 0, spillBuildNullKeys = 0;
  uint64_t joinSpillMatches = 0;
  gxp::HashJoinDesc* devHj = nullptr;
  // AGG_OVER_JOIN: runHashJoin materializes the join output into desc.table,
  // then the fused aggregation runs over it
  bool fusedBindDone = false;
  // decimal columns currently served from DevCol::units (buildDecUnits):
  // fused table / join-agg probe table
  int decUnitsFused = 0, decUnitsJa = 0;
  int lastRowsPerLane = 0;  // gx_debug_rows_per_lane: 0 before any fused pass
  // standalone Selection (compact survivors of a CNF over one source)
  JoinStage selStage;  // probe side only (srcP); hj.post = the CNF
  // standalone Projection (materialize computed columns on device)
  bool projOverSelect = false;
  int projSrcNode = -1;
  gxp::ProjDesc pd;
  gxp::ProjDesc* devPd = nullptr;
  std::vector<int> projOutTypes, projOutFracs;
  std::vector<int> projOutSrcCol;  // >=0 passthrough; -1 computed
  std::vector<int> projOutSprog;   // >=0 string program; -1 otherwise
  std::vector<int> projOutSlot;    // computed: index into pd.out*
  std::vector<int> projOutCat;     // >=0 composed string program (pd.cat)

  ~gx_exec() {
    for (void* p : devBufs) hipFree(p);
    for (void* p : persistBufs) hipFree(p);
    if (hostResult) (void)hipHostFree(hostResult);
    if (evK0) (void)hipEventDestroy(evK0);
    if (evK1) (void)hipEventDestroy(evK1);
  }
};

// ---------------- helpers ----------------

static bool gpuAvailable() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// gxp::MyDecimal -> int128 units at its digitsFrac (requires <= 38 digits)
static bool decToUnits(const MyDecimal& d, __int128* out, int* scale) {
  int wordsInt = (d.digitsInt + 8) / 9;
  int wordsFrac = (d.digitsFrac + 8) / 9;
  if (d.digitsFrac > 9) return false;  // round-1 device scales are <= 9
  __int128 ip = 0;
  for (int i = 0; i < wordsInt; i++) {
    ip = ip * 1000000000 + d.wordBuf[i];
    if (ip > (__int128)1e36) return false;
  }
  static const int64_t p10[10] = {1, 10, 100, 1000, 10000, 100000, 1000000,
                                  10000000, 100000000, 1000000000};
  int64_t fr = 0;
  if (wordsFrac > 0) fr = d.wordBuf[wordsInt] / p10[9 - d.digitsFrac];
  __int128 u = ip * p10[d.digitsFrac] + fr;
  if (d.negative) u = -u;
  *out = u;
  *scale = d.digitsFrac;
  return true;
}

static void setDevColMeta(gxp::DevCol* c, int type, int frac) {
  c->type = type;
  c->frac = frac;
  c->elemSize = type == GX_TYPE_DECIMAL ? 40 : (type == GX_TYPE_STRING ? -1 : 8);
}

// column schema -> table metadata (pointers and row count arrive at run time)
static void setTableMeta(gxp::DevTable* t, const std::vector<int>& types,
                         const std::vector<int>& fracs) {
  t->nCols = (int)types.size();
  for (size_t c = 0; c < types.size(); c++)
    setDevColMeta(&t->cols[c], types[c], fracs[c]);
}

#define HIP_OK(ex, call)                                        \
  do {                                                          \
    hipError_t _e = (call);                                     \
    if (_e != hipSuccess) {                                     \
      (ex)->err = std::string("HIP error: ") + hipGetErrorString(_e); \
      return GX_ERR_INTERNAL;                                   \
    }                                                           \
  } while (0)

static void* devAlloc(gx_exec* ex, size_t n) {
  void* p = nullptr;
  // +16 B slack: glds tail tiles may read a few bytes past the last row
  if (hipMalloc(&p, n + 16) != hipSuccess) return nullptr;
  ex->devBufs.push_back(p);
  return p;
}

static void freeSince(gx_exec* ex, size_t mark) {
  for (size_t i = mark; i < ex->devBufs.size(); i++)
    (void)hipFree(ex->devBufs[i]);
  ex->devBufs.resize(mark);
}

// persistent allocation: survives beginRun/freeSince (pointer is cached in a
// gx_exec field across runs); freed only at destroy
static void* devAllocP(gx_exec* ex, size_t n) {
  void* p = nullptr;
  if (hipMalloc(&p, n + 16) != hipSuccess) return nullptr;
  ex->persistBufs.push_back(p);
  return p;
}

static void devFreeP(gx_exec* ex, void* p) {
  for (size_t i = 0; i < ex->persistBufs.size(); i++)
    if (ex->persistBufs[i] == p) {
      (void)hipFree(p);
      ex->persistBufs.erase(ex->persistBufs.begin() + i);
      return;
    }
}

// per-run allocation scope: the first run records where its allocations
// begin; every re-run (gx_open resets ranQuery) frees them first so repeated
// open/next cycles do not grow device memory. Persistent singletons
// (devErr/devHj/stream/counters) and cached source materializations are
// allocated BEFORE beginRun is called.
static void beginRun(gx_exec* ex) {
  if (ex->runMark == SIZE_MAX)
    ex->runMark = ex->devBufs.size();
  else
    freeSince(ex, ex->runMark);
}

// ---------------- plan compilation ----------------

// composed string calls (CONCAT / CONCAT_WS / CAST_STR): outputs of the
// standalone Projection only, see compileStrCat
static bool isComposedCall(const PExpr& e) {
  return e.kind == EK_CALL && (e.func == GX_F_CONCAT ||
                               e.func == GX_F_CONCAT_WS ||
                               e.func == GX_F_CAST_STR);
}

static bool exprHasComposed(const PPlan& plan, int eid) {
  if (eid < 0 || eid >= (int)plan.exprs.size()) return false;
  const PExpr& e = plan.exprs[eid];
  if (isComposedCall(e)) return true;
  for (int a : e.args)
    if (exprHasComposed(plan, a)) return true;
  return false;
}

static const char* kComposedOverMsg =
    "UPPER/LOWER/SUBSTR/TRIM/LENGTH/LIKE over a CONCAT, CONCAT_WS or CAST_STR "
    "result is unsupported (apply them to the arguments instead)";

// general LIKE / NOT LIKE call (GX_F_LIKE / GX_F_NOT_LIKE): args are
// (string COLUMN, const string pattern [, const i64 escape byte]). Validates
// them against the schema the call runs over and compiles the pattern
// (gx_like.h). colBase = plan colref index of that schema's first column.
static bool compileLikeCall(gx_exec* ex, const PExpr& e,
                            const std::vector<int>& colTypes, int colBase,
                            int* colOut, gxp::LikePat* out) {
  if (e.args.size() != 2 && e.args.size() != 3) {
    ex->err = "LIKE takes (string column, const pattern [, const escape])";
    return false;
  }
  const PExpr& col = ex->plan.exprs[e.args[0]];
  const PExpr& pat = ex->plan.exprs[e.args[1]];
  int c = col.colIdx - colBase;
  if (exprHasComposed(ex->plan, e.args[0])) {
    ex->err = kComposedOverMsg;
    return false;
  }
  if (col.kind != EK_COLREF || c < 0 || c >= (int)colTypes.size() ||
      colTypes[c] != GX_TYPE_STRING) {
    ex->err = "device LIKE: the first argument must be a string column";
    return false;
  }
  if (pat.kind != EK_CONST || pat.retType != GX_TYPE_STRING) {
    ex->err = "device LIKE: the pattern must be a string constant";
    return false;
  }
  int64_t esc = 92;
  if (e.args.size() == 3) {
    const PExpr& ee = ex->plan.exprs[e.args[2]];
    if (ee.kind != EK_CONST || ee.retType != GX_TYPE_I64 || ee.constI64 < 0 ||
        ee.constI64 > 255) {
      ex->err = "device LIKE: the escape must be a constant byte 0..255";
      return false;
    }
    esc = ee.constI64;
  }
  int32_t n = gxp::likeCompilePat((const uint8_t*)pat.constStr.data(),
                                  (int32_t)pat.constStr.size(), (int32_t)esc,
                                  out);
  if (n < 0) {
    ex->err = "device LIKE: the pattern compiles to more than 32 elements";
    return false;
  }
  *colOut = c;
  return true;
}

// value-context LIKE: intern the compiled pattern in a VM_LIKE pattern table
static int internLikePat(gx_exec* ex, gxp::LikePat* tab, int32_t* nTab,
                         const gxp::LikePat& lp) {
  for (int i = 0; i < *nTab; i++)
    if (tab[i].n == lp.n && tab[i].types == lp.types &&
        std::memcmp(tab[i].chars, lp.chars, sizeof lp.chars) == 0)
      return i;
  if (*nTab >= gxp::kMaxLikePats) {
    ex->err = "more than 4 distinct LIKE patterns in value context";
    return -1;
  }
  tab[*nTab] = lp;
  return (*nTab)++;
}

bool ExprBuilder::allowed(gx_exec* ex, int op) const {
  if ((ops >> op) & 1) return true;
  if (op == gxp::VM_LIKE) {
    // a plan error, not a reason to fall back (gx_exec::jaLikeRejected)
    ex->jaLikeRejected = true;
    ex->err = "LIKE in value context is not supported in the "
              "join-aggregate pipeline";
  } else {
    ex->err = "unsupported function on device path";
  }
  return false;
}

// allocate (or reuse) a raw-fetch slot for (kind, col) on the fused desc
static int fetchSlot(gx_exec* ex, int kind, int col) {
  gxp::FusedQueryDesc& d = ex->desc;
  for (int i = 0; i < d.nFetch; i++)
    if (d.fetch[i].kind == kind && d.fetch[i].col == col) return i;
  if (d.nFetch >= gxp::kMaxFetch) return -1;
  d.fetch[d.nFetch] = {kind, col};
  return d.nFetch++;
}

// compile expression exprId over B's schema into B's VM program. Returns the
// result register (>= 0) or -1; *scaleOut = static decimal scale of the value.
static int vmCompile(gx_exec* ex, ExprBuilder& B, int exprId, int* scaleOut) {
  const PExpr& e = ex->plan.exprs[exprId];
  auto cached = B.memo.find(exprId);
  if (cached != B.memo.end()) {
    *scaleOut = cached->second.second;
    return cached->second.first;
  }
  // schema column of a colref expression, or -1
  auto colOf = [&](const PExpr& x) -> int {
    int col = x.kind == EK_COLREF ? x.colIdx - B.colBase : -1;
    return col >= 0 && col < (int)B.colTypes->size() ? col : -1;
  };
  int reg = -1;
  switch (e.kind) {
    case EK_COLREF: {
      int col = colOf(e);
      if (col < 0) {
        ex->err = "bad colref in device expression";
        return -1;
      }
      int t = (*B.colTypes)[col];
      if (t == GX_TYPE_DECIMAL) {
        int frac = (*B.colFracs)[col];
        reg = B.emit(ex, gxp::VM_LOAD_DEC, B.allocRegFresh(), col, frac);
        *scaleOut = frac;
      } else if (t == GX_TYPE_I64) {
        reg = B.emit(ex, gxp::VM_LOAD_I64, B.allocRegFresh(), col, 0);
        *scaleOut = 0;
      } else {
        ex->err = "unsupported colref type in device expression";
        return -1;
      }
      break;
    }
    case EK_CONST: {
      __int128 u = 0;
      int sc = 0;
      if (e.retType == GX_TYPE_DECIMAL) {
        if (!decToUnits(e.constDec, &u, &sc)) {
          ex->err = "const decimal too wide for device path";
          return -1;
        }
      } else if (e.retType == GX_TYPE_I64) {
        u = e.constI64;
        sc = 0;
      } else {
        ex->err = "unsupported const type in device expression";
        return -1;
      }
      if (*B.nConsts >= gxp::kMaxVmConsts) {
        ex->err = "too many consts";
        return -1;
      }
      int ci = (*B.nConsts)++;
      B.constLo[ci] = (int64_t)(uint64_t)u;
      B.constHi[ci] = (int64_t)(u >> 64);
      if (u > (__int128)INT64_MAX || u < (__int128)INT64_MIN)
        *B.wide = 1;  // narrow VM cannot hold this constant
      reg = B.emit(ex, gxp::VM_LOAD_CONST, B.allocReg(), ci, 0);
      *scaleOut = sc;
      break;
    }
    case EK_CALL: {
      if (e.func == GX_F_LENGTH) {  // builtinLengthSig: byte length -> i64
        if (e.args.size() == 1 && exprHasComposed(ex->plan, e.args[0])) {
          ex->err = kComposedOverMsg;
          return -1;
        }
        if (e.args.size() != 1 ||
            ex->plan.exprs[e.args[0]].kind != EK_COLREF) {
          ex->err = "device LENGTH takes one string column";
          return -1;
        }
        int col = colOf(ex->plan.exprs[e.args[0]]);
        if (col < 0 || (*B.colTypes)[col] != GX_TYPE_STRING) {
          ex->err = "device LENGTH argument must be a string column";
          return -1;
        }
        reg = B.emit(ex, gxp::VM_STRLEN, B.allocRegFresh(), col, 0);
        *scaleOut = 0;
        break;
      }
      if (e.func == GX_F_LIKE || e.func == GX_F_NOT_LIKE) {
        // LIKE in value context: i64 0/1, NULL when the string is NULL
        if (!B.allowed(ex, gxp::VM_LIKE)) return -1;
        gxp::LikePat lp;
        int col;
        if (!compileLikeCall(ex, e, *B.colTypes, B.colBase, &col, &lp))
          return -1;
        int pi = internLikePat(ex, B.likePats, B.nLikePats, lp);
        if (pi < 0) return -1;
        reg = B.emit(ex, gxp::VM_LIKE, B.allocReg(), col, pi,
                     e.func == GX_F_NOT_LIKE ? 1 : 0);
        *scaleOut = 0;
        break;
      }
      if (e.func == GX_F_CAST_DEC || e.func == GX_F_CAST_INT ||
          e.func == GX_F_ROUND) {
        // cast family (ProduceDecWithSpecifiedTp / ToInt) and ROUND(x, d)
        // (builtinRoundWithFracDecSig: scale min(d, ret frac)): round
        // half-up from the arg's scale to the target (VM_ROUND_SCALE)
        int sr;
        if (e.func == GX_F_ROUND) {
          if (e.args.size() != 2 ||
              ex->plan.exprs[e.args[1]].kind != EK_CONST ||
              ex->plan.exprs[e.args[1]].constI64 < 0) {
            ex->err = "ROUND takes (expr, const d >= 0) this round";
            return -1;
          }
          sr = (int)std::min<int64_t>(ex->plan.exprs[e.args[1]].constI64,
                                      e.retFrac);
        } else if (e.args.size() != 1) {
          ex->err = "cast takes one argument";
          return -1;
        } else {
          sr = e.func == GX_F_CAST_INT ? 0 : e.retFrac;
        }
        int sa = 0;
        int ra = vmCompile(ex, B, e.args[0], &sa);
        if (ra < 0) return -1;
        *scaleOut = sr;
        if (sr == sa) {
          reg = ra;  // no-op cast: aliases the argument's register
          break;
        }
        reg = B.emit(ex, gxp::VM_ROUND_SCALE, B.allocReg(), ra, sr, sa);
        B.release(e.args[0]);
        break;
      }
      if (e.func == GX_F_ABS && e.args.size() == 1) {
        int sa = 0;
        int ra = vmCompile(ex, B, e.args[0], &sa);
        if (ra < 0) return -1;
        reg = B.emit(ex, gxp::VM_ABS, B.allocReg(), ra, 0);
        B.release(e.args[0]);
        *scaleOut = sa;
        break;
      }
      if (e.func == GX_F_IF && e.args.size() == 3) {
        // builtinIfSig: branches scale-align; the cond keeps its own scale
        int sc2 = 0, sa = 0, sb = 0, tmpA, tmpB;
        int rc2 = vmCompile(ex, B, e.args[0], &sc2);
        if (rc2 < 0) return -1;
        int ra = vmCompile(ex, B, e.args[1], &sa);
        if (ra < 0) return -1;
        int rb = vmCompile(ex, B, e.args[2], &sb);
        if (rb < 0) return -1;
        *scaleOut = B.alignScales(ex, &ra, sa, &rb, sb, &tmpA, &tmpB);
        if (ra < 0 || rb < 0) break;
        reg = B.emit(ex, gxp::VM_IF, B.allocReg(), rc2, ra, rb);
        B.freeTemp(tmpA);
        B.freeTemp(tmpB);
        B.release(e.args[0]);
        B.release(e.args[1]);
        B.release(e.args[2]);
        break;
      }
      if (e.func >= GX_F_YEAR && e.func <= GX_F_SECOND) {
        // YEAR..SECOND: raw CoreTime bits load (nulls tracked by the load) +
        // bitfield extract; only direct TIME columns this round
        int col = e.args.size() == 1 ? colOf(ex->plan.exprs[e.args[0]]) : -1;
        if (col < 0 || (*B.colTypes)[col] != GX_TYPE_TIME) {
          ex->err = "YEAR/MONTH/DAY take a time column";
          return -1;
        }
        int lr = B.emit(ex, gxp::VM_LOAD_I64, B.allocRegFresh(), col, 0);
        if (lr < 0) break;
        reg = B.emit(ex, gxp::VM_TIME_EXTRACT, B.allocReg(), lr,
                     e.func - GX_F_YEAR);
        *scaleOut = 0;
        break;
      }
      if (e.args.size() != 2) {
        ex->err = "unsupported call arity on device";
        return -1;
      }
      int sa = 0, sb = 0, tmpA, tmpB;
      int ra = vmCompile(ex, B, e.args[0], &sa);
      if (ra < 0) return -1;
      int rb = vmCompile(ex, B, e.args[1], &sb);
      if (rb < 0) return -1;
      if (e.func == GX_F_IFNULL || e.func == GX_F_GREATEST ||
          e.func == GX_F_LEAST || e.func <= GX_F_NE) {
        // builtinIfNullSig / builtinGreatest*Sig / builtinLeast*Sig, and
        // the compare family in VALUE context (i64 0/1, NULL on NULL):
        // align operand scales; compares emit VM_CMP with the op in .c
        int op2 = e.func <= GX_F_NE
                      ? gxp::VM_CMP
                      : e.func == GX_F_IFNULL
                            ? gxp::VM_IFNULL
                            : (e.func == GX_F_GREATEST ? gxp::VM_MAX2
                                                       : gxp::VM_MIN2);
        int target = B.alignScales(ex, &ra, sa, &rb, sb, &tmpA, &tmpB);
        if (ra < 0 || rb < 0) break;
        reg = B.emit(ex, op2, B.allocReg(), ra, rb,
                     op2 == gxp::VM_CMP ? e.func : -1);
        B.freeTemp(tmpA);
        B.freeTemp(tmpB);
        *scaleOut = op2 == gxp::VM_CMP ? 0 : target;
      } else if (e.func == GX_F_DIV) {
        if (!B.allowed(ex, gxp::VM_DIV)) return -1;
        // result scale is word-granular (doDiv, mydecimal.go:1170-1215):
        // frac_i word-rounded, fracIncr reduced by the slack, result frac =
        // words(frac1w + frac2w + incr) * 9
        int f1w = (sa + 8) / 9 * 9;
        int f2w = (sb + 8) / 9 * 9;
        int incr = std::max(0, 4 - (f1w - sa) - (f2w - sb));
        int sr = (f1w + f2w + incr + 8) / 9 * 9;
        if (sr > 30) sr = 30;
        int e10 = sb + (sr - sa);
        if (e10 < 0 || e10 > 36) {
          ex->err = "division scale out of device range";
          return -1;
        }
        reg = B.emit(ex, gxp::VM_DIV, B.allocReg(), ra, rb, e10);
        B.hasDiv = true;
        *scaleOut = sr;
      } else if (e.func == GX_F_MUL) {
        reg = B.emit(ex, gxp::VM_MUL, B.allocReg(), ra, rb);
        *scaleOut = sa + sb;
      } else if (e.func == GX_F_PLUS || e.func == GX_F_MINUS) {
        // align scales to max (MySQL add/sub result frac = max(f1,f2))
        *scaleOut = B.alignScales(ex, &ra, sa, &rb, sb, &tmpA, &tmpB);
        if (ra < 0 || rb < 0) break;
        reg = B.emit(ex, e.func == GX_F_PLUS ? gxp::VM_ADD : gxp::VM_SUB,
                     B.allocReg(), ra, rb);
        B.freeTemp(tmpA);
        B.freeTemp(tmpB);
      } else {
        ex->err = "unsupported function on device path";
        return -1;
      }
      B.release(e.args[0]);
      B.release(e.args[1]);
      break;
    }
  }
  if (reg < 0 && ex->err.empty()) ex->err = "expression too large for device VM";
  if (reg >= 0) B.memo[exprId] = {reg, *scaleOut};
  return reg;
}

// What a load-reordering site moves to the front of its stream.
constexpr uint32_t kVmLoadOps = 1u << gxp::VM_LOAD_DEC | 1u << gxp::VM_LOAD_I64;

// The finishing step of every VM site. Moves the instructions whose opcode
// is in `frontOps` to the front of the stream, keeping their order (each dst
// is written once and loads have no dependencies), then fills the
// per-instruction constants insP10 / insMagic and range-checks what indexes
// the tables. Returns the number of instructions moved to the front, or -1
// with ex->err set.
static int finishVmProgram(gx_exec* ex, ExprBuilder& B, uint32_t frontOps) {
  static const int64_t p10h[19] = {1, 10, 100, 1000, 10000, 100000, 1000000,
                                   10000000, 100000000, 1000000000,
                                   10000000000LL, 100000000000LL,
                                   1000000000000LL, 10000000000000LL,
                                   100000000000000LL, 1000000000000000LL,
                                   10000000000000000LL, 100000000000000000LL,
                                   1000000000000000000LL};
  // ceil(2^62 / 10^(9-f)) at index 9-f
  static const uint64_t magich[10] = {
      4611686018427387904ULL, 461168601842738791ULL, 46116860184273880ULL,
      4611686018427388ULL,    461168601842739ULL,    46116860184274ULL,
      4611686018428ULL,       461168601843ULL,       46116860185ULL,
      4611686019ULL};
  int n = *B.nIns;
  gxp::VmIns* front = std::stable_partition(
      B.ins, B.ins + n,
      [&](const gxp::VmIns& in) { return (frontOps >> in.op) & 1; });
  for (int i = 0; i < n; i++) {
    const gxp::VmIns& in = B.ins[i];
    B.insP10[i] = 1;
    B.insMagic[i] = 0;
    if (in.op == gxp::VM_LOAD_DEC) {
      if (in.b < 0 || in.b > 9) {
        ex->err = "decimal scale out of range (frac must be 0..9, got " +
                  std::to_string(in.b) + ")";
        return -1;
      }
      B.insP10[i] = p10h[in.b];
      B.insMagic[i] = magich[9 - in.b];
    } else if (in.op == gxp::VM_SCALE_UP) {
      if (in.b < 0 || in.b > 18) {
        ex->err = "scale shift out of range";
        return -1;
      }
      B.insP10[i] = p10h[in.b];
    } else if (in.op == gxp::VM_ROUND_SCALE) {
      int sh = in.b - in.c;
      if (sh < -18 || sh > 18) {
        ex->err = "rescale shift out of range";
        return -1;
      }
      B.insP10[i] = p10h[sh >= 0 ? sh : -sh];
    }
  }
  return (int)(front - B.ins);
}

// compile one Selection condition over a single-table schema into a PredDesc
static bool compileTablePred(gx_exec* ex, const PNode& srcNode, int condId,
                             gxp::PredDesc* out, uint8_t* strConst,
                             int32_t* strConstLen) {
  const PExpr& e = ex->plan.exprs[condId];
  if (e.kind == EK_CALL && (e.func == GX_F_LIKE || e.func == GX_F_NOT_LIKE)) {
    // general LIKE: the compiled pattern travels inside the PredDesc
    gxp::LikePat lp;
    int col;
    if (!compileLikeCall(ex, e, srcNode.colTypes, 0, &col, &lp)) return false;
    gxp::PredDesc pd{};
    pd.kind = gxp::PRED_STR_LIKE;
    pd.col = col;
    pd.cmp = e.func == GX_F_LIKE ? GX_F_EQ : GX_F_NE;
    pd.slot = -1;
    std::memcpy(pd.strC, lp.chars, sizeof lp.chars);
    pd.strCLen = lp.n;
    pd.constU64 = lp.types;
    *out = pd;
    return true;
  }
  if (e.kind == EK_CALL && e.func == GX_F_LIKE_PREFIX && e.args.size() == 2) {
    // LIKE 'abc%' fast path (builtinLikeSig): byte prefix, no PAD trimming
    const PExpr& col = ex->plan.exprs[e.args[0]];
    const PExpr& pat = ex->plan.exprs[e.args[1]];
    if (col.kind != EK_COLREF || pat.kind != EK_CONST ||
        col.colIdx < 0 || col.colIdx >= (int)srcNode.colTypes.size() ||
        srcNode.colTypes[col.colIdx] != GX_TYPE_STRING ||
        pat.constStr.size() > 16) {
      ex->err = "device LIKE takes <string column> LIKE <'prefix%' <= 16B>";
      return false;
    }
    gxp::PredDesc pd{};
    pd.kind = gxp::PRED_STR_LIKE_PREFIX;
    pd.col = col.colIdx;
    pd.cmp = GX_F_EQ;
    pd.slot = -1;
    std::memcpy(strConst, pat.constStr.data(), pat.constStr.size());
    *strConstLen = (int32_t)pat.constStr.size();
    *out = pd;
    return true;
  }
  if (e.kind == EK_CALL &&
      (e.func == GX_F_IS_NULL || e.func == GX_F_IS_NOT_NULL) &&
      e.args.size() == 1) {
    // builtin*IsNullSig: the null bit is the value (never NULL itself)
    const PExpr& a0 = ex->plan.exprs[e.args[0]];
    if (a0.kind != EK_COLREF || a0.colIdx < 0 ||
        a0.colIdx >= (int)srcNode.colTypes.size()) {
      ex->err = "IS NULL takes a column";
      return false;
    }
    gxp::PredDesc pd{};
    pd.kind = gxp::PRED_IS_NULL;
    pd.col = a0.colIdx;
    pd.cmp = e.func == GX_F_IS_NULL ? GX_F_EQ : GX_F_NE;
    pd.slot = -1;
    *out = pd;
    return true;
  }
  if (e.kind != EK_CALL || e.func > GX_F_NE || e.args.size() != 2) {
    ex->err = "unsupported filter expression on device";
    return false;
  }
  const PExpr* lhs = &ex->plan.exprs[e.args[0]];
  const PExpr* rhs = &ex->plan.exprs[e.args[1]];
  int cmp = e.func;
  if (lhs->kind == EK_CONST && rhs->kind == EK_COLREF) {
    std::swap(lhs, rhs);
    static const int mirror[6] = {GX_F_GT, GX_F_GE, GX_F_LT, GX_F_LE, GX_F_EQ,
                                  GX_F_NE};
    cmp = mirror[cmp];
  }
  if (lhs->kind != EK_COLREF || rhs->kind != EK_CONST) {
    ex->err = "device filter must be <column> <cmp> <const>";
    return false;
  }
  gxp::PredDesc pd{};
  pd.col = lhs->colIdx;
  pd.cmp = cmp;
  pd.slot = -1;
  if (pd.col < 0 || pd.col >= (int)srcNode.colTypes.size()) {
    ex->err = "filter column out of range";
    return false;
  }
  int ct = srcNode.colTypes[pd.col];
  if (ct == GX_TYPE_TIME && rhs->retType == GX_TYPE_TIME) {
    pd.kind = gxp::PRED_TIME_CMP_CONST;
    pd.constU64 = rhs->constTime;
  } else if (ct == GX_TYPE_I64 && rhs->retType == GX_TYPE_I64) {
    pd.kind = gxp::PRED_I64_CMP_CONST;
    pd.constU64 = (uint64_t)rhs->constI64;
  } else if (ct == GX_TYPE_DECIMAL && rhs->retType == GX_TYPE_DECIMAL) {
    // units compare at the column's declared frac (evalSimplePred loads
    // the narrow decimal; wider-than-i64 consts are out of device range)
    __int128 u;
    int sc;
    if (!decToUnits(rhs->constDec, &u, &sc)) {
      ex->err = "filter const decimal too wide";
      return false;
    }
    int colFrac = srcNode.colFracs[pd.col];
    while (sc < colFrac) {
      u *= 10;
      sc++;
    }
    if (sc != colFrac || u > INT64_MAX || u < INT64_MIN) {
      ex->err = "filter decimal const/scale unsupported";
      return false;
    }
    pd.kind = gxp::PRED_DEC_CMP_CONST;
    pd.constU64 = (uint64_t)(int64_t)u;
  } else if (ct == GX_TYPE_STRING && rhs->retType == GX_TYPE_STRING &&
             (cmp == GX_F_EQ || cmp == GX_F_NE)) {
    if (rhs->constStr.size() > 16) {
      ex->err = "string const too long for device filter";
      return false;
    }
    pd.kind = gxp::PRED_STR_EQ_CONST;
    // PAD SPACE: trim the constant's trailing spaces too
    std::string k = rhs->constStr;
    while (!k.empty() && k.back() == ' ') k.pop_back();
    std::memcpy(strConst, k.data(), k.size());
    *strConstLen = (int32_t)k.size();
  } else {
    ex->err = "unsupported filter column/const type combination";
    return false;
  }
  *out = pd;
  return true;
}

// unwrap [Selection ->] Source; returns source node id (or -1) and the
// selection node (or nullptr)
// full-sort (TOPN limit<0) wrappers below joins/aggregates do not change
// their results -- the merge-join plan shape sorts its inputs on the join
// keys (merge_join.go); the device pipeline hashes instead, so skip them
static int skipFullSort(const PPlan& plan, int node) {
  while (plan.nodes[node].kind == PK_TOPN && plan.nodes[node].limit < 0)
    node = plan.nodes[node].child;
  return node;
}
static int skipFullSort(gx_exec* ex, int node) {
  return skipFullSort(ex->plan, node);
}

static int unwrapSource(gx_exec* ex, int node, const PNode** selOut) {
  *selOut = nullptr;
  node = skipFullSort(ex, node);
  const PNode* n = &ex->plan.nodes[node];
  if (n->kind == PK_SELECTION) {
    *selOut = n;
    node = n->child;
    node = skipFullSort(ex, node);
    n = &ex->plan.nodes[node];
  }
  if (n->kind != PK_SOURCE) return -1;
  return node;
}

// recognize & compile the join-aggregate (Q3-class) plan:
// TopN <- HashAgg(sum) <- Projection <- HashJoin(probe=lineitem,
//   build=HashJoin(build=customer, probe=orders))
static int32_t compileJoinAgg(gx_exec* ex, int topnNode) {
  const PPlan& plan = ex->plan;
  const PNode& topn = plan.nodes[topnNode];
  if (topn.limit <= 0 || topn.limit + topn.offset > 100000) {
    ex->err = "device TopN limit too large";
    return GX_ERR_INVALID;
  }
  const PNode& agg = plan.nodes[topn.child];
  if (agg.kind != PK_HASHAGG || agg.aggMode != GX_AGG_MODE_COMPLETE ||
      agg.aggFuncs.size() != 1 || agg.aggFuncs[0] != GX_AGG_SUM ||
      agg.exprs.empty() || agg.exprs.size() > 3) {
    ex->err = "unsupported aggregate shape for device join path";
    return GX_ERR_INVALID;
  }
  const PNode& proj = plan.nodes[agg.child];
  if (proj.kind != PK_PROJECTION) {
    ex->err = "expected projection under aggregate";
    return GX_ERR_INVALID;
  }
  const PNode& j2 = plan.nodes[skipFullSort(ex, proj.child)];
  if ((j2.kind != PK_HASHJOIN && j2.kind != PK_MERGEJOIN) ||
      j2.joinType != 0 || j2.buildKeys.size() != 1) {
    ex->err = "unsupported join shape";
    return GX_ERR_INVALID;
  }
  const PNode& j1 = plan.nodes[skipFullSort(ex, j2.child)];
  if ((j1.kind != PK_HASHJOIN && j1.kind != PK_MERGEJOIN) ||
      j1.joinType != 0 || j1.buildKeys.size() != 1) {
    ex->err = "unsupported inner join shape";
    return GX_ERR_INVALID;
  }
  const PNode *selC, *selO, *selL;
  int srcC = unwrapSource(ex, j1.child, &selC);
  int srcO = unwrapSource(ex, j1.child2, &selO);
  int srcL = unwrapSource(ex, j2.child2, &selL);
  if (srcC < 0 || srcO < 0 || srcL < 0) {
    ex->err = "join children must be [Selection ->] Source";
    return GX_ERR_INVALID;
  }
  const PNode& custN = plan.nodes[srcC];
  const PNode& ordN = plan.nodes[srcO];
  const PNode& liN = plan.nodes[srcL];
  int nc = (int)custN.colTypes.size();
  int no = (int)ordN.colTypes.size();
  gxp::JoinAggDesc& ja = ex->ja;

  // join keys (single-column int64)
  const PExpr& bk1 = plan.exprs[j1.buildKeys[0]];
  const PExpr& pk1 = plan.exprs[j1.probeKeys[0]];
  const PExpr& bk2 = plan.exprs[j2.buildKeys[0]];
  const PExpr& pk2 = plan.exprs[j2.probeKeys[0]];
  if (bk1.kind != EK_COLREF || pk1.kind != EK_COLREF || bk2.kind != EK_COLREF ||
      pk2.kind != EK_COLREF) {
    ex->err = "join keys must be columns";
    return GX_ERR_INVALID;
  }
  if (custN.colTypes[bk1.colIdx] != GX_TYPE_I64 ||
      ordN.colTypes[pk1.colIdx] != GX_TYPE_I64 ||
      liN.colTypes[pk2.colIdx] != GX_TYPE_I64 || bk2.colIdx < nc ||
      bk2.colIdx >= nc + no || ordN.colTypes[bk2.colIdx - nc] != GX_TYPE_I64) {
    ex->err = "device join keys must be int64";
    return GX_ERR_INVALID;
  }
  ja.b0KeyCol = bk1.colIdx;
  ja.b1ProbeCol = pk1.colIdx;
  ja.b1KeyCol = bk2.colIdx - nc;
  ja.pKeyCol = pk2.colIdx;

  // predicates: 1-4 CNF conjuncts per table (the first is specialized into
  // the tuned kernels/JIT; extras evaluate through the evalSimplePred loop)
  auto doPred = [&](const PNode* sel, const PNode& srcNode, gxp::PredDesc* pd,
                    int32_t* n, gxp::PredDesc* px, int32_t* nx) -> bool {
    *n = 0;
    *nx = 0;
    if (!sel) return true;
    if (sel->exprs.empty() || sel->exprs.size() > 4) {
      ex->err = "device join path supports 1-4 filter conjuncts per table";
      return false;
    }
    for (size_t j = 0; j < sel->exprs.size(); j++) {
      gxp::PredDesc* dst = j == 0 ? pd : &px[j - 1];
      int32_t before = ja.strConstLen;
      if (!compileTablePred(ex, srcNode, sel->exprs[j], dst, ja.strConst,
                            &ja.strConstLen))
        return false;
      if ((dst->kind == gxp::PRED_STR_EQ_CONST ||
           dst->kind == gxp::PRED_STR_LIKE_PREFIX) &&
          before != 0) {
        // one shared 16-byte string constant per join-agg plan this round
        ex->err = "one string filter constant per device join-agg plan";
        return false;
      }
    }
    *n = 1;
    *nx = (int32_t)sel->exprs.size() - 1;
    return true;
  };
  if (!doPred(selC, custN, &ja.pred0, &ja.nPred0, ja.pred0x, &ja.nPred0x))
    return GX_ERR_INVALID;
  if (!doPred(selO, ordN, &ja.pred1, &ja.nPred1, ja.pred1x, &ja.nPred1x))
    return GX_ERR_INVALID;
  if (!doPred(selL, liN, &ja.predP, &ja.nPredP, ja.predPx, &ja.nPredPx))
    return GX_ERR_INVALID;

  // projection classification
  ja.payloadCol0 = ja.payloadCol1 = -1;
  std::vector<int> projClass(proj.exprs.size(), -1);  // 0 probekey 1 pay0 2 pay1 3 value
  int valueExpr = -1;
  for (size_t i = 0; i < proj.exprs.size(); i++) {
    const PExpr& pe = plan.exprs[proj.exprs[i]];
    if (pe.kind == EK_COLREF) {
      if (pe.colIdx >= nc + no) {
        int lcol = pe.colIdx - nc - no;
        if (lcol == ja.pKeyCol) projClass[i] = 0;
        else {
          ex->err = "probe-side passthrough must be the join key";
          return GX_ERR_INVALID;
        }
      } else if (pe.colIdx >= nc) {
        int ocol = pe.colIdx - nc;
        int t = ordN.colTypes[ocol];
        if (t != GX_TYPE_I64 && t != GX_TYPE_TIME) {
          ex->err = "payload columns must be 8-byte";
          return GX_ERR_INVALID;
        }
        if (ja.payloadCol0 < 0 || ja.payloadCol0 == ocol) {
          ja.payloadCol0 = ocol;
          projClass[i] = 1;
        } else if (ja.payloadCol1 < 0 || ja.payloadCol1 == ocol) {
          ja.payloadCol1 = ocol;
          projClass[i] = 2;
        } else {
          ex->err = "too many build payload columns";
          return GX_ERR_INVALID;
        }
      } else {
        ex->err = "customer-side payload not supported this round";
        return GX_ERR_INVALID;
      }
    } else {
      if (valueExpr >= 0) {
        ex->err = "one computed value per device join";
        return GX_ERR_INVALID;
      }
      valueExpr = proj.exprs[i];
      projClass[i] = 3;
    }
  }
  if (valueExpr < 0) {
    ex->err = "missing value expression";
    return GX_ERR_INVALID;
  }
  // the agg arg must be the value expr; group cols map through projClass
  const PExpr& aggArg = plan.exprs[agg.aggArgs[0]];
  if (aggArg.kind != EK_COLREF || projClass[aggArg.colIdx] != 3) {
    ex->err = "sum argument must be the computed value";
    return GX_ERR_INVALID;
  }
  ex->jaGroupSrc.clear();
  ex->jaGroupType.clear();
  for (int ge : agg.exprs) {
    const PExpr& gexpr = plan.exprs[ge];
    if (gexpr.kind != EK_COLREF || projClass[gexpr.colIdx] < 0 ||
        projClass[gexpr.colIdx] == 3) {
      ex->err = "group keys must be the join key or payload columns";
      return GX_ERR_INVALID;
    }
    int cls = projClass[gexpr.colIdx];
    ex->jaGroupSrc.push_back(cls);
    if (cls == 0) ex->jaGroupType.push_back(GX_TYPE_I64);
    else if (cls == 1) ex->jaGroupType.push_back(ordN.colTypes[ja.payloadCol0]);
    else ex->jaGroupType.push_back(ordN.colTypes[ja.payloadCol1]);
  }

  // value expression VM over the probe (lineitem) table; the probe kernel
  // runs the core opcode set
  ExprBuilder B;
  B.bind(ja, &liN.colTypes, &liN.colFracs, nc + no, gxp::kVmOpsCore,
         kVmRegsNarrowState);
  int sc = 0;
  int reg = vmCompile(ex, B, valueExpr, &sc);
  if (reg < 0) return GX_ERR_INVALID;
  ja.valueReg = reg;
  ex->jaValueScale = sc;
  // lazy value loads: only the FILTER column is prefetched — the VM runs
  // only for rows that pass the filter AND hit the hash table (a small
  // fraction), so its columns are loaded at use (ins.c = -1)
  if (ja.nPredP &&
      (ja.predP.kind == gxp::PRED_TIME_CMP_CONST ||
       ja.predP.kind == gxp::PRED_I64_CMP_CONST)) {
    ja.fetch[0] = {gxp::FETCH_8B, ja.predP.col};
    ja.nFetch = 1;
    ja.predP.slot = 0;
  }
  // loads first (mirrors the fused path)
  if (finishVmProgram(ex, B, kVmLoadOps) < 0) return GX_ERR_INVALID;

  // topn keys -> positions in the agg output row [groups..., sum]
  ex->jaSortKeys.clear();
  int aggWidth = (int)agg.exprs.size() + 1;
  for (size_t i = 0; i < topn.exprs.size(); i++) {
    const PExpr& ke = plan.exprs[topn.exprs[i]];
    if (ke.kind != EK_COLREF || ke.colIdx < 0 || ke.colIdx >= aggWidth) {
      ex->err = "TopN keys must be aggregate output columns";
      return GX_ERR_INVALID;
    }
    ex->jaSortKeys.push_back({ke.colIdx, topn.keyDesc[i] != 0});
  }
  ex->jaLimit = topn.limit;
  ex->jaOffset = topn.offset;
  ex->jaSrcCust = srcC;
  ex->jaSrcOrd = srcO;
  ex->jaSrcLi = srcL;
  ex->jaAggFrac = agg.aggFracs[0];
  return GX_OK;
}

// ---------------- standalone hash join compilation (stage model) ----------
// A join subtree (nested joins allowed) compiles bottom-up into
// gx_exec::joinStages: each stage is one HashJoinV2-equivalent
// (join/hash_join_v2.go) whose sides are bound sources ([Selection ->]
// Source) or previous stages' materialized output tables.

static int32_t compileJoinStage(gx_exec* ex, int joinNode,
                                const PNode* postSel, int* stageOut);

struct JoinSideRef {
  int srcNode = -1;            // bound source (-1 if stage-fed)
  int stage = -1;              // feeding stage (-1 if source)
  const PNode* sel = nullptr;  // Selection over a SOURCE side (table pred)
  std::vector<int> types, fracs;
};

static int32_t resolveJoinSide(gx_exec* ex, int node, JoinSideRef* side) {
  node = skipFullSort(ex, node);
  const PNode* n = &ex->plan.nodes[node];
  if (n->kind == PK_SELECTION) {
    const PNode* sel = n;
    int child = skipFullSort(ex, n->child);
    const PNode* cn = &ex->plan.nodes[child];
    if (cn->kind == PK_HASHJOIN) {
      // the selection is the inner join\'s post filter (other conditions)
      int st = -1;
      int32_t rc = compileJoinStage(ex, child, sel, &st);
      if (rc) return rc;
      side->stage = st;
      side->types = ex->joinStages[st].types;
      side->fracs = ex->joinStages[st].fracs;
      return GX_OK;
    }
    if (cn->kind != PK_SOURCE) {
      ex->err = "join children must be [Selection ->] Source or a join";
      return GX_ERR_INVALID;
    }
    side->srcNode = child;
    side->sel = sel;
    side->types = cn->colTypes;
    side->fracs = cn->colFracs;
    return GX_OK;
  }
  if (n->kind == PK_HASHJOIN) {
    int st = -1;
    int32_t rc = compileJoinStage(ex, node, nullptr, &st);
    if (rc) return rc;
    side->stage = st;
    side->types = ex->joinStages[st].types;
    side->fracs = ex->joinStages[st].fracs;
    return GX_OK;
  }
  if (n->kind == PK_SOURCE) {
    side->srcNode = node;
    side->types = n->colTypes;
    side->fracs = n->colFracs;
    return GX_OK;
  }
  ex->err = "join children must be [Selection ->] Source or a join";
  return GX_ERR_INVALID;
}

// post-join filter conjuncts (a Selection over the join = the join\'s "other
// conditions", inner_join_probe.go:75): <output col cmp const> or
// <output col cmp output col> (e.g. build.x < probe.y)
static int32_t compilePostJoinPreds(gx_exec* ex, const PNode& sel,
                                    const std::vector<int>& outTypes,
                                    const std::vector<int>& outFracs, int nb,
                                    gxp::HashJoinDesc& hj) {
  const PPlan& plan = ex->plan;
  if (sel.exprs.size() > 4) {
    ex->err = "too many post-join filter conjuncts this round";
    return GX_ERR_INVALID;
  }
  PNode outN;
  outN.colTypes = outTypes;
  outN.colFracs = outFracs;
  // each top-level conjunct may be a disjunction: flatten OR trees into
  // leaf predicates; the group head records how many follow (orWith)
  std::vector<int> leaves;
  std::function<bool(int)> flatten = [&](int cid) {
    const PExpr& ee = plan.exprs[cid];
    if (ee.kind == EK_CALL && ee.func == GX_F_OR && ee.args.size() == 2)
      return flatten(ee.args[0]) && flatten(ee.args[1]);
    leaves.push_back(cid);
    return true;
  };
  for (int condId : sel.exprs) {
    leaves.clear();
    if (!flatten(condId)) return GX_ERR_INVALID;
    if (hj.nPost + (int)leaves.size() > 8) {
      ex->err = "too many filter predicates after OR flattening";
      return GX_ERR_INVALID;
    }
    int groupHead = hj.nPost;
  for (int cid : leaves) {
    const PExpr& e = plan.exprs[cid];
    gxp::JoinPostPred q{};
    bool colcol = e.kind == EK_CALL && e.args.size() == 2 &&
                  e.func != GX_F_LIKE && e.func != GX_F_NOT_LIKE &&
                  plan.exprs[e.args[0]].kind == EK_COLREF &&
                  plan.exprs[e.args[1]].kind == EK_COLREF;
    if (colcol) {
      if (e.func > GX_F_NE) {
        ex->err = "unsupported post-join predicate";
        return GX_ERR_INVALID;
      }
      const PExpr& l = plan.exprs[e.args[0]];
      const PExpr& r = plan.exprs[e.args[1]];
      if (l.colIdx < 0 || l.colIdx >= (int)outN.colTypes.size() ||
          r.colIdx < 0 || r.colIdx >= (int)outN.colTypes.size()) {
        ex->err = "post-join filter column out of range";
        return GX_ERR_INVALID;
      }
      int lt = outN.colTypes[l.colIdx], rt = outN.colTypes[r.colIdx];
      if (lt != rt || (lt != GX_TYPE_I64 && lt != GX_TYPE_TIME)) {
        ex->err = "post-join col-col compare supports int64/time this round";
        return GX_ERR_INVALID;
      }
      q.kind = 1;
      q.lcol = l.colIdx;
      q.rcol = r.colIdx;
      q.cmp = e.func;
      q.ctype = lt;
    } else {
      if (!compileTablePred(ex, outN, cid, &q.pd, q.strC, &q.strCLen))
        return GX_ERR_INVALID;
      q.kind = 0;
      q.side = q.pd.col < nb ? 0 : 1;
      if (q.side == 1) q.pd.col -= nb;
    }
    hj.post[hj.nPost++] = q;
  }
    hj.post[groupHead].orWith = (int32_t)(hj.nPost - groupHead - 1);
  }
  return GX_OK;
}

static int32_t compileJoinStage(gx_exec* ex, int joinNode,
                                const PNode* postSel, int* stageOut) {
  const PPlan& plan = ex->plan;
  const PNode& jn = plan.nodes[joinNode];
  if (jn.joinType < 0 || jn.joinType > 7) {
    ex->err = "unsupported join type (0=inner, 1=left outer, 2=right outer, "
              "3=semi, 4=anti semi, 5=null-aware anti semi, 6=left outer "
              "semi, 7=null-aware left outer semi)";
    return GX_ERR_INVALID;
  }
  if (jn.buildKeys.size() != jn.probeKeys.size() || jn.buildKeys.empty() ||
      (int)jn.buildKeys.size() > gxp::kMaxJoinKeys) {
    ex->err = "too many join key columns";
    return GX_ERR_INVALID;
  }
  JoinSideRef B, P;
  int32_t rc = resolveJoinSide(ex, jn.child, &B);
  if (rc) return rc;
  rc = resolveJoinSide(ex, jn.child2, &P);
  if (rc) return rc;
  int nb = (int)B.types.size();
  int np = (int)P.types.size();
  if (nb + np > gxp::kMaxCols) {
    ex->err = "too many join output columns";
    return GX_ERR_INVALID;
  }
  gx_exec::JoinStage st;
  gxp::HashJoinDesc& hj = st.hj;
  hj.joinType = jn.joinType;
  hj.nKeys = (int32_t)jn.buildKeys.size();
  for (int k = 0; k < hj.nKeys; k++) {
    const PExpr& bk = plan.exprs[jn.buildKeys[k]];
    const PExpr& pk = plan.exprs[jn.probeKeys[k]];
    if (bk.kind != EK_COLREF || pk.kind != EK_COLREF || bk.colIdx < 0 ||
        bk.colIdx >= nb || pk.colIdx < 0 || pk.colIdx >= np) {
      ex->err = "join keys must be child columns";
      return GX_ERR_INVALID;
    }
    int bt = B.types[bk.colIdx];
    int pt = P.types[pk.colIdx];
    // SerializeKeys semantics (codec.go:852-910): int64/packed-Time compare
    // as their raw 8 bytes; decimals compare value-normalized (ToHashKey,
    // so 1.10 == 1.1 across fracs); strings compare PAD-SPACE-trimmed bytes
    if (bt != pt) {
      ex->err = "join key column types must match";
      return GX_ERR_INVALID;
    }
    if (bt == GX_TYPE_I64 || bt == GX_TYPE_TIME) {
      hj.keyKind[k] = 0;
    } else if (bt == GX_TYPE_DECIMAL) {
      hj.keyKind[k] = 1;
      hj.generalKeys = 1;
    } else if (bt == GX_TYPE_STRING) {
      hj.keyKind[k] = 2;
      hj.generalKeys = 1;
    } else {
      ex->err = "unsupported join key column type";
      return GX_ERR_INVALID;
    }
    hj.bKeyCol[k] = bk.colIdx;
    hj.pKeyCol[k] = pk.colIdx;
  }
  if (hj.nKeys > 2) hj.generalKeys = 1;  // fast path caches 2 u64 keys
  // one filter conjunct per SOURCE side (stage-fed sides carry their filter
  // as the inner stage\'s post preds)
  auto doPred = [&](const PNode* sel, int srcNode, gxp::PredDesc* pd,
                    int32_t* n, uint8_t* sc, int32_t* scLen) -> bool {
    *n = 0;
    if (!sel) return true;
    if (sel->exprs.size() != 1) {
      ex->err = "device join path supports one filter conjunct per table";
      return false;
    }
    if (!compileTablePred(ex, ex->plan.nodes[srcNode], sel->exprs[0], pd, sc,
                          scLen))
      return false;
    *n = 1;
    return true;
  };
  if (!doPred(B.sel, B.srcNode, &hj.predB, &hj.nPredB, hj.strConstB,
              &hj.strConstBLen))
    return GX_ERR_INVALID;
  if (!doPred(P.sel, P.srcNode, &hj.predP, &hj.nPredP, hj.strConstP,
              &hj.strConstPLen))
    return GX_ERR_INVALID;
  st.srcB = B.srcNode;
  st.srcP = P.srcNode;
  st.buildStage = B.stage;
  st.probeStage = P.stage;
  if (jn.joinType >= 3) {
    // semi family emits the probe side only; the left-outer-semi forms
    // (6/7) append the x IN (...) scalar as a trailing i64 column
    st.types = P.types;
    st.fracs = P.fracs;
    if (jn.joinType >= 6) {
      st.types.push_back(GX_TYPE_I64);
      st.fracs.push_back(0);
    }
  } else {
    st.types = B.types;
    st.fracs = B.fracs;
    st.types.insert(st.types.end(), P.types.begin(), P.types.end());
    st.fracs.insert(st.fracs.end(), P.fracs.begin(), P.fracs.end());
  }
  if (postSel) {
    if (jn.joinType != 0) {
      // other conditions change which outer rows count as matched
      // (outer_join_probe.go post-condition matched tracking) — not wired
      // into the non-inner paths yet; fail loudly rather than mis-join
      ex->err = "post-join conditions with non-inner joins unsupported this round";
      return GX_ERR_INVALID;
    }
    rc = compilePostJoinPreds(ex, *postSel, st.types, st.fracs, nb, hj);
    if (rc) return rc;
  }
  ex->joinStages.push_back(std::move(st));
  *stageOut = (int)ex->joinStages.size() - 1;
  return GX_OK;
}

// [Selection ->] HashJoin subtree (the Selection = post-join other
// conditions); nested joins compile into stages, root stage last
static int32_t compileHashJoinTree(gx_exec* ex, int node) {
  const PNode* n = &ex->plan.nodes[node];
  const PNode* sel = nullptr;
  if (n->kind == PK_SELECTION) {
    sel = n;
    node = n->child;
    n = &ex->plan.nodes[node];
  }
  if (n->kind != PK_HASHJOIN) {
    ex->err = "expected a hash join under the selection";
    return GX_ERR_INVALID;
  }
  int root = -1;
  int32_t rc = compileJoinStage(ex, node, sel, &root);
  if (rc) return rc;
  // root stage must be last (bottom-up compile order guarantees it)
  gx_exec::JoinStage& st = ex->joinStages[root];
  setTableMeta(&ex->desc.table, st.types, st.fracs);
  return GX_OK;
}

// standalone Selection over a Source (SelectionExec, select.go:750-785):
// survivors compact on device, columns gather through the survivor index
static int32_t compileSelect(gx_exec* ex, int selNode) {
  const PNode& sel = ex->plan.nodes[selNode];
  int child = skipFullSort(ex, sel.child);
  const PNode& srcN = ex->plan.nodes[child];
  if (srcN.kind != PK_SOURCE) {
    ex->err = "selection child must be a source";
    return GX_ERR_INVALID;
  }
  if ((int)srcN.colTypes.size() > gxp::kMaxCols) {
    ex->err = "too many source columns";
    return GX_ERR_INVALID;
  }
  gx_exec::JoinStage& st = ex->selStage;
  st.srcP = child;
  st.types = srcN.colTypes;
  st.fracs = srcN.colFracs;
  int32_t rc = compilePostJoinPreds(ex, sel, st.types, st.fracs, 0, st.hj);
  if (rc) return rc;
  setTableMeta(&ex->desc.table, st.types, st.fracs);
  return GX_OK;
}

// recognize a {SUBSTR, UPPER}* chain over a string column and fold it into
// one StrProg (windows compose; ASCII upcase commutes with windowing)
static bool compileStrProg(gx_exec* ex, int exprId,
                           const std::vector<int>& types, gxp::StrProg* sp) {
  const PExpr& e = ex->plan.exprs[exprId];
  if (e.kind == EK_COLREF) {
    if (e.colIdx < 0 || e.colIdx >= (int)types.size() ||
        types[e.colIdx] != GX_TYPE_STRING)
      return false;
    sp->col = e.colIdx;
    return true;
  }
  if (e.kind != EK_CALL) return false;
  if ((e.func == GX_F_UPPER || e.func == GX_F_LOWER) && e.args.size() == 1) {
    if (!compileStrProg(ex, e.args[0], types, sp)) return false;
    // ASCII case ops: the OUTERMOST call decides (lower(upper(x)) == lower(x))
    sp->upper = e.func == GX_F_UPPER;
    sp->lower = e.func == GX_F_LOWER;
    return true;
  }
  if (e.func == GX_F_TRIM && e.args.size() == 1) {
    if (!compileStrProg(ex, e.args[0], types, sp)) return false;
    if (sp->nWin >= gxp::kMaxStrWin) return false;
    sp->winPos[sp->nWin] = 0;
    sp->winLen[sp->nWin] = -1;  // trim pseudo-window
    sp->nWin++;
    return true;
  }
  if (e.func == GX_F_SUBSTR && e.args.size() == 3) {
    if (!compileStrProg(ex, e.args[0], types, sp)) return false;
    const PExpr& p = ex->plan.exprs[e.args[1]];
    const PExpr& l = ex->plan.exprs[e.args[2]];
    if (p.kind != EK_CONST || l.kind != EK_CONST ||
        sp->nWin >= gxp::kMaxStrWin)
      return false;
    sp->winPos[sp->nWin] = p.constI64;
    sp->winLen[sp->nWin] = l.constI64;
    sp->nWin++;
    return true;
  }
  return false;
}

// ---- composed string outputs (CONCAT / CONCAT_WS / CAST_STR, gx_strcat.h) ----

// composed strings exist only as outputs of the root Projection: anywhere
// else in the tree (group, join and sort keys, predicates, aggregate
// arguments, inner projections) they are a plan error
static bool composedOnlyAtRootProjection(gx_exec* ex) {
  const PPlan& plan = ex->plan;
  std::vector<int> todo{ex->root};
  std::set<int> seen;
  while (!todo.empty()) {
    int ni = todo.back();
    todo.pop_back();
    if (ni < 0 || ni >= (int)plan.nodes.size() || !seen.insert(ni).second)
      continue;
    const PNode& n = plan.nodes[ni];
    todo.push_back(n.child);
    todo.push_back(n.child2);
    if (ni == ex->root && n.kind == PK_PROJECTION) continue;
    bool bad = false;
    for (const std::vector<int>* v :
         {&n.exprs, &n.aggArgs, &n.buildKeys, &n.probeKeys})
      for (int eid : *v) bad = bad || exprHasComposed(plan, eid);
    if (bad) {
      ex->err = "CONCAT / CONCAT_WS / CAST_STR are valid only as outputs of "
                "the standalone Projection over [Selection ->] Source: not "
                "as group keys, join keys, sort keys, aggregate arguments or "
                "predicates";
      return false;
    }
  }
  return true;
}

// a constant into the operator's pool
static bool catAddConst(gx_exec* ex, gxp::ProjDesc& pd, const std::string& s,
                        uint16_t* off, uint16_t* len) {
  if ((size_t)pd.catPoolLen + s.size() > (size_t)gxp::kStrCatPoolBytes) {
    ex->err = "more than 256 bytes of string constants in one projection "
              "(CONCAT / CONCAT_WS constants, separators included)";
    return false;
  }
  std::memcpy(pd.catPool + pd.catPoolLen, s.data(), s.size());
  *off = (uint16_t)pd.catPoolLen;
  *len = (uint16_t)s.size();
  pd.catPoolLen += (int32_t)s.size();
  return true;
}

static bool catNewPiece(gx_exec* ex, gxp::StrCatProg* cp, gxp::StrPiece** out) {
  if (cp->nPieces >= gxp::kStrCatMaxPieces) {
    ex->err = "more than 8 pieces in one CONCAT / CONCAT_WS output (after "
              "flattening nested CONCATs)";
    return false;
  }
  *out = &cp->piece[cp->nPieces++];
  **out = gxp::StrPiece{};
  return true;
}

// CAST_STR(x): x is an i64 column (read in place) or an expression the
// projection VM compiles to an i64, materialized as a hidden computed output
static bool catAddCast(gx_exec* ex, ExprBuilder& B, gxp::ProjDesc& pd,
                       const std::vector<int>& types, const PExpr& e,
                       gxp::StrCatProg* cp) {
  static const char* kArgMsg =
      "CAST_STR takes one signed integer argument (decimal, float, time, "
      "string and unsigned arguments are rejected)";
  if (e.args.size() != 1) {
    ex->err = kArgMsg;
    return false;
  }
  const PExpr& a = ex->plan.exprs[e.args[0]];
  bool i64 = a.retType == GX_TYPE_I64;
  if (a.kind == EK_COLREF)
    i64 = a.colIdx >= 0 && a.colIdx < (int)types.size() &&
          types[a.colIdx] == GX_TYPE_I64;
  if (!i64) {
    ex->err = kArgMsg;
    return false;
  }
  gxp::StrPiece* pc;
  if (!catNewPiece(ex, cp, &pc)) return false;
  pc->kind = gxp::SPK_I64;
  if (a.kind == EK_COLREF) {
    pc->col = (int16_t)a.colIdx;
    return true;
  }
  int sc = 0;
  int reg = vmCompile(ex, B, e.args[0], &sc);
  if (reg < 0) {
    if (ex->err.empty()) ex->err = "unsupported CAST_STR argument expression";
    return false;
  }
  if (sc != 0) {
    ex->err = kArgMsg;
    return false;
  }
  if (pd.nOut >= gxp::kMaxCols) {
    ex->err = "too many computed outputs (a computed CAST_STR argument is a "
              "hidden one; 16 per projection)";
    return false;
  }
  int o = pd.nOut++;
  pd.outReg[o] = reg;
  pd.outScale[o] = 0;
  pd.outType[o] = GX_TYPE_I64;
  pc->slot = (int16_t)o;
  return true;
}

// one argument of CONCAT / CONCAT_WS -> piece(s) of cp
static bool catAddArg(gx_exec* ex, ExprBuilder& B, gxp::ProjDesc& pd,
                      const std::vector<int>& types, int argId,
                      gxp::StrCatProg* cp) {
  const PExpr& a = ex->plan.exprs[argId];
  if (a.kind == EK_CONST) {
    if (a.retType != GX_TYPE_STRING) {
      ex->err = "CONCAT / CONCAT_WS arguments are strings (wrap an integer "
                "in CAST_STR)";
      return false;
    }
    gxp::StrPiece* pc;
    if (!catNewPiece(ex, cp, &pc)) return false;
    pc->kind = gxp::SPK_CONST;
    return catAddConst(ex, pd, a.constStr, &pc->constOff, &pc->constLen);
  }
  if (a.kind == EK_CALL && a.func == GX_F_CAST_STR)
    return catAddCast(ex, B, pd, types, a, cp);
  if (a.kind == EK_CALL && a.func == GX_F_CONCAT_WS) {
    ex->err = "CONCAT_WS nested inside CONCAT or CONCAT_WS is unsupported";
    return false;
  }
  if (a.kind == EK_CALL && a.func == GX_F_CONCAT) {
    if (cp->ws) {  // the NULL rules differ: it would not flatten
      ex->err = "CONCAT nested inside CONCAT_WS is unsupported (a nested "
                "CONCAT flattens inside CONCAT only)";
      return false;
    }
    if (a.args.empty()) {
      ex->err = "CONCAT takes at least one argument";
      return false;
    }
    for (int sub : a.args)
      if (!catAddArg(ex, B, pd, types, sub, cp)) return false;
    return true;
  }
  gxp::StrProg sp{};
  if (!compileStrProg(ex, argId, types, &sp)) {
    // name the limit when the chain bottoms out in a composed string
    int cur = argId;
    while (ex->plan.exprs[cur].kind == EK_CALL &&
           !isComposedCall(ex->plan.exprs[cur]) &&
           !ex->plan.exprs[cur].args.empty())
      cur = ex->plan.exprs[cur].args[0];
    ex->err = isComposedCall(ex->plan.exprs[cur])
                  ? kComposedOverMsg
                  : "unsupported CONCAT / CONCAT_WS argument (a string column "
                    "under SUBSTR/UPPER/LOWER/TRIM, a constant string, "
                    "CAST_STR, or a nested CONCAT)";
    return false;
  }
  gxp::StrPiece* pc;
  if (!catNewPiece(ex, cp, &pc)) return false;
  pc->kind = gxp::SPK_WINDOW;
  pc->col = (int16_t)sp.col;
  pc->caseOp = sp.upper ? gxp::SCO_UPPER
                        : (sp.lower ? gxp::SCO_LOWER : gxp::SCO_NONE);
  pc->nWin = (uint8_t)sp.nWin;
  for (int w = 0; w < sp.nWin; w++) {
    pc->winPos[w] = gxp::strWinSaturate(sp.winPos[w]);
    pc->winLen[w] = gxp::strWinSaturate(sp.winLen[w]);
  }
  return true;
}

// a CONCAT / CONCAT_WS / CAST_STR projection output -> one StrCatProg
static bool compileStrCat(gx_exec* ex, ExprBuilder& B, gxp::ProjDesc& pd,
                          const std::vector<int>& types, int exprId,
                          gxp::StrCatProg* cp) {
  const PExpr& e = ex->plan.exprs[exprId];
  *cp = gxp::StrCatProg{};
  if (e.func == GX_F_CAST_STR) return catAddCast(ex, B, pd, types, e, cp);
  size_t first = 0;
  if (e.func == GX_F_CONCAT_WS) {
    if (e.args.size() < 2) {
      ex->err = "CONCAT_WS takes a separator and at least one argument";
      return false;
    }
    const PExpr& sep = ex->plan.exprs[e.args[0]];
    if (sep.kind != EK_CONST || sep.retType != GX_TYPE_STRING) {
      ex->err = "the CONCAT_WS separator must be a constant string";
      return false;
    }
    cp->ws = 1;
    if (!catAddConst(ex, pd, sep.constStr, &cp->sepOff, &cp->sepLen))
      return false;
    first = 1;
  } else if (e.args.empty()) {
    ex->err = "CONCAT takes at least one argument";
    return false;
  }
  for (size_t i = first; i < e.args.size(); i++)
    if (!catAddArg(ex, B, pd, types, e.args[i], cp)) return false;
  return true;
}

// standalone Projection over a Source or a Selection(Source)
// (ProjectionExec, projection.go:77): computed expressions materialize as
// device columns (decimal encode on device), passthrough colrefs alias the
// input buffers
static int32_t compileProject(gx_exec* ex, int projNode) {
  const PPlan& plan = ex->plan;
  const PNode& pj = plan.nodes[projNode];
  int childNode = skipFullSort(ex, pj.child);
  const PNode* cn = &plan.nodes[childNode];
  const std::vector<int>* childTypes;
  const std::vector<int>* childFracs;
  if (cn->kind == PK_SELECTION &&
      plan.nodes[skipFullSort(ex, cn->child)].kind == PK_SOURCE) {
    int32_t rc = compileSelect(ex, childNode);
    if (rc) return rc;
    ex->projOverSelect = true;
    childTypes = &ex->selStage.types;
    childFracs = &ex->selStage.fracs;
  } else if (cn->kind == PK_SOURCE) {
    ex->projSrcNode = childNode;
    childTypes = &cn->colTypes;
    childFracs = &cn->colFracs;
  } else {
    ex->err = "projection child must be [Selection ->] Source";
    return GX_ERR_INVALID;
  }
  if ((int)pj.exprs.size() > gxp::kMaxCols) {
    ex->err = "too many projection outputs";
    return GX_ERR_INVALID;
  }
  gxp::ProjDesc& pd = ex->pd;
  ExprBuilder B;
  B.bind(pd, childTypes, childFracs, 0, kVmOpsProject, kVmRegsNarrowState);
  B.bindLikePats(pd);
  for (int eid : pj.exprs) {
    const PExpr& e = plan.exprs[eid];
    if (e.kind == EK_COLREF) {
      if (e.colIdx < 0 || e.colIdx >= (int)childTypes->size()) {
        ex->err = "projection column out of range";
        return GX_ERR_INVALID;
      }
      ex->projOutSrcCol.push_back(e.colIdx);
      ex->projOutSlot.push_back(-1);
      ex->projOutSprog.push_back(-1);
      ex->projOutTypes.push_back((*childTypes)[e.colIdx]);
      ex->projOutFracs.push_back((*childFracs)[e.colIdx]);
    } else if (isComposedCall(e)) {
      // composed string outputs: pieces of several columns, constants and
      // integer text (gx_strcat.h)
      if (pd.nCat >= gxp::kMaxCols ||
          !compileStrCat(ex, B, pd, *childTypes, eid, &pd.cat[pd.nCat])) {
        if (ex->err.empty()) ex->err = "unsupported composed string projection";
        return GX_ERR_INVALID;
      }
      ex->projOutSrcCol.push_back(-1);
      ex->projOutSlot.push_back(-1);
      ex->projOutSprog.push_back(-1);
      ex->projOutTypes.push_back(GX_TYPE_STRING);
      ex->projOutFracs.push_back(0);
      ex->projOutCat.resize(ex->projOutTypes.size(), -1);
      ex->projOutCat.back() = pd.nCat++;
    } else if (e.kind == EK_CALL && e.retType == GX_TYPE_STRING) {
      // string outputs: SUBSTR/UPPER chains fold into one windowed view
      gxp::StrProg sp{};
      if (!compileStrProg(ex, eid, *childTypes, &sp)) {
        int cur = eid;
        while (ex->plan.exprs[cur].kind == EK_CALL &&
               !isComposedCall(ex->plan.exprs[cur]) &&
               !ex->plan.exprs[cur].args.empty())
          cur = ex->plan.exprs[cur].args[0];
        ex->err = isComposedCall(ex->plan.exprs[cur])
                      ? kComposedOverMsg
                      : "unsupported string projection (SUBSTR/UPPER/LOWER/"
                        "TRIM chains over a string column, or CONCAT / "
                        "CONCAT_WS / CAST_STR of such chains, constants and "
                        "integers)";
        return GX_ERR_INVALID;
      }
      int si = pd.nSprog++;
      pd.sprog[si] = sp;
      ex->projOutSrcCol.push_back(-1);
      ex->projOutSlot.push_back(-1);
      ex->projOutSprog.push_back(si);
      ex->projOutTypes.push_back(GX_TYPE_STRING);
      ex->projOutFracs.push_back(0);
    } else {
      int sc = 0;
      int reg = vmCompile(ex, B, eid, &sc);
      if (reg < 0) {
        if (ex->err.empty()) ex->err = "unsupported projection expression";
        return GX_ERR_INVALID;
      }
      int outType = e.retType == GX_TYPE_I64 ? GX_TYPE_I64 : GX_TYPE_DECIMAL;
      if (pd.nOut >= gxp::kMaxCols) {  // hidden CAST_STR arguments count too
        ex->err = "too many computed outputs (a computed CAST_STR argument is "
                  "a hidden one; 16 per projection)";
        return GX_ERR_INVALID;
      }
      int o = pd.nOut++;
      pd.outReg[o] = reg;
      pd.outScale[o] = sc;
      pd.outType[o] = outType;
      ex->projOutSrcCol.push_back(-1);
      ex->projOutSlot.push_back(o);
      ex->projOutSprog.push_back(-1);
      ex->projOutTypes.push_back(outType);
      ex->projOutFracs.push_back(outType == GX_TYPE_I64 ? 0 : sc);
    }
  }
  ex->projOutCat.resize(ex->projOutTypes.size(), -1);
  // the projection kernel loads directly, in program order (no fetch
  // pipeline, no reorder)
  if (finishVmProgram(ex, B, 0) < 0) return GX_ERR_INVALID;
  // OUTPUT schema for emission
  setTableMeta(&ex->desc.table, ex->projOutTypes, ex->projOutFracs);
  return GX_OK;
}

static int32_t compileFused(gx_exec* ex, int aggNode);

static const char kHavingErr[] =
    "unsupported HAVING condition (col cmp const, IS NULL, OR of those)";

// append the in-order leaves of one HAVING conjunct: <agg output col cmp
// const> or IS [NOT] NULL(col), composed with LogicOr; col indexes bound by
// the aggregate's USER output width
static bool havingLeaves(const PPlan& plan, int cid, int width,
                         gxp::HavingCond* out) {
  const PExpr& e = plan.exprs[cid];
  if (e.kind != EK_CALL) return false;
  if (e.func == GX_F_OR && e.args.size() == 2)
    return havingLeaves(plan, e.args[0], width, out) &&
           havingLeaves(plan, e.args[1], width, out);
  gxp::HavingLeaf leaf;
  const PExpr* col;
  if ((e.func == GX_F_IS_NULL || e.func == GX_F_IS_NOT_NULL) &&
      e.args.size() == 1) {
    leaf.isNullTest = true;
    leaf.wantNull = e.func == GX_F_IS_NULL;
    col = &plan.exprs[e.args[0]];
  } else {
    if (e.func < 0 || e.func > GX_F_NE || e.args.size() != 2) return false;
    col = &plan.exprs[e.args[0]];
    const PExpr* cst = &plan.exprs[e.args[1]];
    leaf.cmp = e.func;
    if (col->kind == EK_CONST && cst->kind == EK_COLREF) {
      std::swap(col, cst);
      static const int mirror[6] = {GX_F_GT, GX_F_GE, GX_F_LT, GX_F_LE,
                                    GX_F_EQ, GX_F_NE};
      leaf.cmp = mirror[e.func];
    }
    if (cst->kind != EK_CONST) return false;
    leaf.cst.type = cst->retType;
    leaf.cst.i64 = cst->constI64;
    leaf.cst.u64 = cst->constTime;
    leaf.cst.f64 = cst->constF64;
    leaf.cst.dec = cst->constDec;
    leaf.cst.str = cst->constStr;
  }
  if (col->kind != EK_COLREF || col->colIdx < 0 || col->colIdx >= width)
    return false;
  leaf.col = col->colIdx;
  out->push_back(std::move(leaf));
  return true;
}

// HAVING shape rules, once, at build: the Selection's conjuncts over the
// output of aggregate `an` become ex->having. Whether a leaf's value and
// constant types pair is checked at decode, when the leaf is reached.
static bool compileHaving(gx_exec* ex, const std::vector<int>& conds,
                          const PNode& an) {
  int width = (int)(an.exprs.size() + an.aggFuncs.size());
  ex->having.clear();
  for (int cid : conds) {
    ex->having.emplace_back();
    if (!havingLeaves(ex->plan, cid, width, &ex->having.back())) {
      ex->err = kHavingErr;
      return false;
    }
  }
  return true;
}

// general aggregation over joined rows: HashAgg <- [Projection] <-
// [Selection] <- HashJoin. The join materializes its output table on device
// (runHashJoin), then the fused aggregation kernel runs over that table —
// the generalization of the Q3-class fused pipeline to arbitrary aggregate
// shapes (at the cost of materializing the joined columns once).
static int32_t compileAggOverJoin(gx_exec* ex, int aggNode) {
  PPlan& plan = ex->plan;
  // walk down to the join, remembering the agg-side chain
  std::vector<int> chain;  // aggNode first, bottom-most last
  int node = aggNode;
  while (plan.nodes[node].kind == PK_HASHAGG ||
         plan.nodes[node].kind == PK_PROJECTION ||
         plan.nodes[node].kind == PK_SELECTION) {
    chain.push_back(node);
    node = plan.nodes[node].child;
  }
  if (plan.nodes[node].kind != PK_HASHJOIN) {
    ex->err = "expected a hash join under the aggregation";
    return GX_ERR_INVALID;
  }
  int32_t rc = compileHashJoinTree(ex, node);
  if (rc) return rc;
  // pseudo source carrying the join output schema (root stage)
  PNode ps;
  ps.kind = PK_SOURCE;
  ps.colTypes = ex->joinStages.back().types;
  ps.colFracs = ex->joinStages.back().fracs;
  plan.nodes.push_back(ps);
  int cur = (int)plan.nodes.size() - 1;
  // clone the agg-side chain bottom-up with the join replaced by the pseudo
  // source (clones, so the original plan stays intact)
  for (int i = (int)chain.size() - 1; i >= 0; i--) {
    PNode copy = plan.nodes[chain[i]];
    copy.child = cur;
    plan.nodes.push_back(copy);
    cur = (int)plan.nodes.size() - 1;
  }
  // the fused desc's table metadata is overwritten from the pseudo source;
  // actual column pointers/nRows arrive when runHashJoin materializes
  return compileFused(ex, cur);
}

// compile the fused Source->[Selection]->[Projection]->HashAgg pipeline
static int32_t compileFused(gx_exec* ex, int aggNode) {
  // DISTINCT rewrite: aggregate over DISTINCT values == group by
  // (keys..., arg) on the device (the dedup falls out of the group table),
  // then fold on the host at decode. All aggs must be DISTINCT over ONE
  // shared arg this round; the inner device agg becomes count(*) (unused).
  {
    PNode& aggN = ex->plan.nodes[aggNode];
    bool anyD = false;
    for (int f : aggN.aggFuncs) anyD |= f >= GX_AGG_COUNT_DISTINCT;
    if (anyD) {
      if (aggN.aggMode != GX_AGG_MODE_COMPLETE) {
        ex->err = "DISTINCT aggregates support COMPLETE mode only";
        return GX_ERR_INVALID;
      }
      std::vector<int> argExprs;  // appended inner keys, deduped
      std::vector<std::vector<int>> slotOf(aggN.aggFuncs.size());
      auto slotFor = [&](int argE) {
        // share one inner key per distinct ARG: same expr id, or two
        // colrefs naming the same column
        for (size_t p = 0; p < argExprs.size(); p++) {
          const PExpr& x = ex->plan.exprs[argExprs[p]];
          const PExpr& y = ex->plan.exprs[argE];
          if (argExprs[p] == argE ||
              (x.kind == EK_COLREF && y.kind == EK_COLREF &&
               x.colIdx == y.colIdx && x.retType == y.retType))
            return (int)p;
        }
        argExprs.push_back(argE);
        return (int)argExprs.size() - 1;
      };
      for (size_t a = 0; a < aggN.aggFuncs.size(); a++) {
        int argE = aggN.aggArgs[a];
        if (aggN.aggFuncs[a] < GX_AGG_COUNT_DISTINCT || argE < 0) {
          ex->err = "DISTINCT aggregates cannot mix with plain aggregates "
                    "this round";
          return GX_ERR_INVALID;
        }
        const PExpr& ae = ex->plan.exprs[argE];
        if (ae.kind == EK_CALL && ae.func == GX_F_TUPLE) {
          // multi-column distinct (count(distinct a, b, ...)): each tuple
          // element becomes an inner key; the fold excludes rows with ANY
          // NULL element
          if (aggN.aggFuncs[a] != GX_AGG_COUNT_DISTINCT || ae.args.empty()) {
            ex->err = "tuple args take COUNT DISTINCT only";
            return GX_ERR_INVALID;
          }
          for (int el : ae.args) slotOf[a].push_back(slotFor(el));
          continue;
        }
        if (aggN.aggFuncs[a] != GX_AGG_COUNT_DISTINCT &&
            ae.retType != GX_TYPE_DECIMAL) {
          ex->err = "SUM/AVG DISTINCT takes a decimal arg (cast ints)";
          return GX_ERR_INVALID;
        }
        slotOf[a].push_back(slotFor(argE));
      }
      ex->distinct.funcs = aggN.aggFuncs;
      ex->distinct.fracs = aggN.aggFracs;
      ex->distinct.argSlot = slotOf;
      ex->distinct.nKeys = (int)aggN.exprs.size();
      for (int e : argExprs) aggN.exprs.push_back(e);
      aggN.aggFuncs.assign(1, GX_AGG_COUNT);
      aggN.aggArgs.assign(1, -1);
      aggN.aggFracs.assign(1, 0);
    }
  }
  const PPlan& plan = ex->plan;
  ex->aggRoot = aggNode;
  const PNode* agg = &plan.nodes[aggNode];
  const PNode* proj = nullptr;
  const PNode* sel = nullptr;
  const PNode* src = nullptr;
  const PNode* cur = &plan.nodes[agg->child];
  if (cur->kind == PK_PROJECTION) {
    proj = cur;
    cur = &plan.nodes[cur->child];
  }
  if (cur->kind == PK_SELECTION) {
    sel = cur;
    cur = &plan.nodes[cur->child];
  }
  if (cur->kind != PK_SOURCE) {
    ex->err = "unsupported plan shape for device execution "
              "(want HashAgg <- [Projection] <- [Selection] <- Source)";
    return GX_ERR_INVALID;
  }
  src = cur;
  ex->sourceNode = (int)(src - plan.nodes.data());

  // source schema -> desc.table metadata (pointers at open)
  if ((int)src->colTypes.size() > gxp::kMaxCols) {
    ex->err = "too many source columns";
    return GX_ERR_INVALID;
  }
  setTableMeta(&ex->desc.table, src->colTypes, src->colFracs);

  // selection -> PredDescs (CNF of OR groups: each conjunct may be a
  // LogicOr tree of simple predicates, flattened with orWith group heads)
  if (sel) {
    std::vector<int> fusedLeaves;
    std::function<void(int)> fusedFlatten = [&](int cid) {
      const PExpr& fe = plan.exprs[cid];
      if (fe.kind == EK_CALL && fe.func == GX_F_OR && fe.args.size() == 2) {
        fusedFlatten(fe.args[0]);
        fusedFlatten(fe.args[1]);
      } else {
        fusedLeaves.push_back(cid);
      }
    };
    for (int topCond : sel->exprs) {
      fusedLeaves.clear();
      fusedFlatten(topCond);
      int groupHead = ex->desc.nPreds;
    for (int condId : fusedLeaves) {
      const PExpr& e = plan.exprs[condId];
      if (e.kind == EK_CALL &&
          (e.func == GX_F_LIKE || e.func == GX_F_NOT_LIKE)) {
        // general LIKE in the fused CNF: same PredDesc as every other site
        if (ex->desc.nPreds >= gxp::kMaxPreds) {
          ex->err = "too many filter conjuncts";
          return GX_ERR_INVALID;
        }
        gxp::PredDesc pd{};
        if (!compileTablePred(ex, *src, condId, &pd, nullptr, nullptr))
          return GX_ERR_INVALID;
        ex->desc.preds[ex->desc.nPreds++] = pd;
        continue;
      }
      if (e.kind == EK_CALL && e.func == GX_F_LIKE_PREFIX &&
          e.args.size() == 2) {
        // LIKE 'abc%' in the fused CNF (byte prefix, no PAD trimming)
        const PExpr& col = plan.exprs[e.args[0]];
        const PExpr& pat = plan.exprs[e.args[1]];
        if (col.kind != EK_COLREF || pat.kind != EK_CONST ||
            col.colIdx < 0 || col.colIdx >= (int)src->colTypes.size() ||
            src->colTypes[col.colIdx] != GX_TYPE_STRING ||
            pat.constStr.size() > 16) {
          ex->err = "device LIKE takes <string column> LIKE <'prefix%' <= 16B>";
          return GX_ERR_INVALID;
        }
        if (ex->desc.nPreds >= gxp::kMaxPreds) {
          ex->err = "too many filter conjuncts";
          return GX_ERR_INVALID;
        }
        gxp::PredDesc pd{};
        pd.kind = gxp::PRED_STR_LIKE_PREFIX;
        pd.col = col.colIdx;
        pd.cmp = GX_F_EQ;
        pd.slot = -1;
        std::memcpy(pd.strC, pat.constStr.data(), pat.constStr.size());
        pd.strCLen = (int32_t)pat.constStr.size();
        ex->desc.preds[ex->desc.nPreds++] = pd;
        continue;
      }
      if (e.kind == EK_CALL &&
          (e.func == GX_F_IS_NULL || e.func == GX_F_IS_NOT_NULL) &&
          e.args.size() == 1) {
        const PExpr& a0 = plan.exprs[e.args[0]];
        if (a0.kind != EK_COLREF || a0.colIdx < 0 ||
            a0.colIdx >= (int)src->colTypes.size()) {
          ex->err = "IS NULL takes a column";
          return GX_ERR_INVALID;
        }
        if (ex->desc.nPreds >= gxp::kMaxPreds) {
          ex->err = "too many filter conjuncts";
          return GX_ERR_INVALID;
        }
        gxp::PredDesc pd{};
        pd.kind = gxp::PRED_IS_NULL;
        pd.col = a0.colIdx;
        pd.cmp = e.func == GX_F_IS_NULL ? GX_F_EQ : GX_F_NE;
        pd.slot = -1;
        ex->desc.preds[ex->desc.nPreds++] = pd;
        continue;
      }
      if (e.kind != EK_CALL || e.func > GX_F_NE || e.args.size() != 2) {
        ex->err = "unsupported filter expression on device";
        return GX_ERR_INVALID;
      }
      const PExpr* lhs = &plan.exprs[e.args[0]];
      const PExpr* rhs = &plan.exprs[e.args[1]];
      int cmp = e.func;
      if (lhs->kind == EK_CONST && rhs->kind == EK_COLREF) {
        std::swap(lhs, rhs);
        // mirror the comparison
        static const int mirror[6] = {GX_F_GT, GX_F_GE, GX_F_LT, GX_F_LE,
                                      GX_F_EQ, GX_F_NE};
        cmp = mirror[cmp];
      }
      if (lhs->kind != EK_COLREF || rhs->kind != EK_CONST) {
        ex->err = "device filter must be <column> <cmp> <const>";
        return GX_ERR_INVALID;
      }
      if (ex->desc.nPreds >= gxp::kMaxPreds) {
        ex->err = "too many filter conjuncts";
        return GX_ERR_INVALID;
      }
      gxp::PredDesc pd{};
      pd.col = lhs->colIdx;
      pd.cmp = cmp;
      int ct = src->colTypes[lhs->colIdx];
      pd.slot = -1;
      if (ct == GX_TYPE_TIME && rhs->retType == GX_TYPE_TIME) {
        pd.kind = gxp::PRED_TIME_CMP_CONST;
        pd.constU64 = rhs->constTime;
        pd.slot = fetchSlot(ex, gxp::FETCH_8B, lhs->colIdx);
        if (pd.slot < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
      } else if (ct == GX_TYPE_I64 && rhs->retType == GX_TYPE_I64) {
        pd.kind = gxp::PRED_I64_CMP_CONST;
        pd.constU64 = (uint64_t)rhs->constI64;
        pd.slot = fetchSlot(ex, gxp::FETCH_8B, lhs->colIdx);
        if (pd.slot < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
      } else if (ct == GX_TYPE_DECIMAL && rhs->retType == GX_TYPE_DECIMAL) {
        __int128 u;
        int sc;
        if (!decToUnits(rhs->constDec, &u, &sc)) {
          ex->err = "filter const decimal too wide";
          return GX_ERR_INVALID;
        }
        // align const to the column's declared frac
        int colFrac = src->colFracs[lhs->colIdx];
        while (sc < colFrac) {
          u *= 10;
          sc++;
        }
        if (sc != colFrac || u > INT64_MAX || u < INT64_MIN) {
          ex->err = "filter decimal const/scale unsupported";
          return GX_ERR_INVALID;
        }
        pd.kind = gxp::PRED_DEC_CMP_CONST;
        pd.constU64 = (uint64_t)(int64_t)u;
        pd.slot = fetchSlot(ex, gxp::FETCH_DEC16, lhs->colIdx);
      } else if (ct == GX_TYPE_STRING && rhs->retType == GX_TYPE_STRING &&
                 (cmp == GX_F_EQ || cmp == GX_F_NE) &&
                 rhs->constStr.size() <= 16) {
        // string EQ/NE const in the fused CNF (PAD SPACE: trim the
        // constant's trailing spaces like the column's, collate.go:272)
        pd.kind = gxp::PRED_STR_EQ_CONST;
        std::string k = rhs->constStr;
        while (!k.empty() && k.back() == ' ') k.pop_back();
        std::memcpy(pd.strC, k.data(), k.size());
        pd.strCLen = (int32_t)k.size();
      } else {
        ex->err = "unsupported filter column/const type combination";
        return GX_ERR_INVALID;
      }
      ex->desc.preds[ex->desc.nPreds++] = pd;
    }
      if (ex->desc.nPreds > groupHead)
        ex->desc.preds[groupHead].orWith =
            (int32_t)(ex->desc.nPreds - groupHead - 1);
    }
  }

  // the expression compiler for this attempt (an earlier failed attempt's
  // state goes with it): full opcode set, registers recycled below the
  // projection outputs the aggregates read
  ex->vm = ExprBuilder{};
  ex->vm.bind(ex->desc, &src->colTypes, &src->colFracs, 0, gxp::kVmOpsFull,
              gxp::kMaxVmRegs);
  ex->vm.bindLikePats(ex->desc);
  {
    std::vector<int> roots;
    if (proj) {
      roots = proj->exprs;
    } else {
      for (int a : agg->aggArgs)
        if (a >= 0) roots.push_back(a);
    }
    ex->vm.countConsumers(plan, roots);
  }

  // projection exprs -> VM registers (group-col projections stay colrefs)
  std::vector<int> projSrcCol;  // proj idx -> source col for passthroughs
  ex->projRegs.clear();
  if (proj) {
    for (int pe : proj->exprs) {
      const PExpr& e = plan.exprs[pe];
      if (e.kind == EK_COLREF &&
          (src->colTypes[e.colIdx] == GX_TYPE_STRING ||
           src->colTypes[e.colIdx] == GX_TYPE_TIME)) {
        projSrcCol.push_back(e.colIdx);
        ex->projRegs.push_back({-1, 0});
        continue;
      }
      int sc = 0;
      int reg = vmCompile(ex, ex->vm, pe, &sc);
      if (reg < 0) return GX_ERR_INVALID;
      projSrcCol.push_back(e.kind == EK_COLREF ? e.colIdx : -1);
      ex->projRegs.push_back({reg, sc});
    }
  }

  // group keys — two device paths (gx_common.h GroupKeyDesc): the packed u64
  // key for <= 2 dense-char/short-string/small-i64 columns (the Q1 shape,
  // JIT-supported), and the serialized wide-key path (codec.HashGroupKey
  // semantics, util/codec/codec.go:1791-1879) for arbitrary column sets —
  // strings of any length, decimals, time, up to kMaxGroupKeyCols columns.
  // Decimal/time keys and >2 columns force wide at compile; strings decide
  // packed-vs-wide at bind (offset density known there); packed-lane overflow
  // at run time (string > 3 B, i64 >= 2^31) converts to wide and reruns.
  gxp::GroupKeyDesc gk{};
  gk.nCols = 0;
  bool forceWideKeys = (int)agg->exprs.size() > 2;
  for (int ge : agg->exprs) {
    const PExpr& e = plan.exprs[ge];
    int srcCol = -1;
    bool computed = false;  // projection-computed key (e.g. YEAR(t))
    if (e.kind != EK_COLREF) {
      ex->err = "group-by expression must be a column";
      return GX_ERR_INVALID;
    }
    if (proj) {
      if (e.colIdx >= (int)projSrcCol.size()) {
        ex->err = "group-by column out of range";
        return GX_ERR_INVALID;
      }
      if (projSrcCol[e.colIdx] >= 0) srcCol = projSrcCol[e.colIdx];
      else computed = true;
    } else {
      srcCol = e.colIdx;
    }
    if (gk.nCols >= gxp::kMaxGroupKeyCols) {
      ex->err = "too many group-by key columns";
      return GX_ERR_INVALID;
    }
    if (computed) {
      // computed i64/decimal group key (GROUP BY YEAR(t), a+b, ...): the
      // value lives in a stable VM register; wide keys hash/record it at
      // its compile-time scale (kind 4)
      const PExpr& pe = plan.exprs[proj->exprs[e.colIdx]];
      if (pe.retType != GX_TYPE_I64 && pe.retType != GX_TYPE_DECIMAL) {
        ex->err = "computed group keys are i64/decimal this round";
        return GX_ERR_INVALID;
      }
      forceWideKeys = true;
      int sc = 0;
      int reg = vmCompile(ex, ex->vm, proj->exprs[e.colIdx], &sc);
      if (reg < 0) {
        if (ex->err.empty()) ex->err = "group key compile failed";
        return GX_ERR_INVALID;
      }
      // col < 0 marks a computed key; -2 = i64 result, -1 = decimal
      gk.col[gk.nCols] = pe.retType == GX_TYPE_I64 ? -2 : -1;
      gk.kind[gk.nCols] = 4;
      gk.slot[gk.nCols] = reg;
      gk.kscale[gk.nCols] = sc;
      gk.nCols++;
      continue;
    }
    int t = src->colTypes[srcCol];
    gk.col[gk.nCols] = srcCol;
    gk.kscale[gk.nCols] = 0;
    if (t == GX_TYPE_STRING) {
      gk.kind[gk.nCols] = 0;   // bind refines: dense -> 2, else packed 0/wide 5
      gk.slot[gk.nCols] = -1;  // slot at open (density known)
    } else if (t == GX_TYPE_I64) {
      gk.kind[gk.nCols] = 1;   // bind flips to 3 (raw 8B) in wide mode
      gk.slot[gk.nCols] = fetchSlot(ex, gxp::FETCH_8B, srcCol);
      if (gk.slot[gk.nCols] < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
    } else if (t == GX_TYPE_TIME) {
      forceWideKeys = true;
      gk.kind[gk.nCols] = 3;
      gk.slot[gk.nCols] = fetchSlot(ex, gxp::FETCH_8B, srcCol);
      if (gk.slot[gk.nCols] < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
    } else if (t == GX_TYPE_DECIMAL) {
      forceWideKeys = true;
      int sc = 0;
      // loaded through the VM (canonical units at the column's static scale;
      // load registers are never recycled, so the register is stable)
      int srcExpr = proj ? proj->exprs[e.colIdx] : ge;
      int reg = vmCompile(ex, ex->vm, srcExpr, &sc);
      if (reg < 0) {
        if (ex->err.empty()) ex->err = "group key compile failed";
        return GX_ERR_INVALID;
      }
      gk.kind[gk.nCols] = 4;
      gk.slot[gk.nCols] = reg;
      gk.kscale[gk.nCols] = sc;
    } else {
      ex->err = "unsupported group key column type";
      return GX_ERR_INVALID;
    }
    gk.nCols++;
  }
  gk.wideMode = forceWideKeys ? 1 : 0;
  ex->desc.gkey = gk;

  // aggs
  if ((int)agg->aggFuncs.size() > gxp::kMaxAggs) {
    ex->err = "too many aggregates";
    return GX_ERR_INVALID;
  }
  for (size_t a = 0; a < agg->aggFuncs.size(); a++) {
    gxp::AggDesc ad{};
    ad.func = agg->aggFuncs[a];
    if (ad.func == GX_AGG_FIRSTROW) {
      // the golden Q1 plan carries firstrow(group col) (§8d): its value is
      // fully determined by the group key, so it needs no per-row state
      int argE = agg->aggArgs[a];
      int srcCol = -1;
      if (argE >= 0 && plan.exprs[argE].kind == EK_COLREF) {
        int ci = plan.exprs[argE].colIdx;
        if (proj) {
          if (ci < (int)projSrcCol.size()) srcCol = projSrcCol[ci];
        } else {
          srcCol = ci;
        }
      }
      for (int k = 0; k < gk.nCols; k++)
        if (srcCol >= 0 && gk.col[k] == srcCol) ad.fr = k;
      if (ad.fr < 0) {
        ex->err = "device firstrow supports group-by columns this round";
        return GX_ERR_INVALID;
      }
      ad.srcReg = -1;
      ad.scale = 0;
      ex->desc.aggs[ex->desc.nAggs++] = ad;
      continue;
    }
    if (ad.func != GX_AGG_COUNT && ad.func != GX_AGG_SUM &&
        ad.func != GX_AGG_AVG && ad.func != GX_AGG_MIN &&
        ad.func != GX_AGG_MAX) {
      ex->err = "device aggregation supports count/sum/avg/min/max this round";
      return GX_ERR_INVALID;
    }
    int argE = agg->aggArgs[a];
    if (argE < 0) {
      ad.srcReg = -1;
      ad.scale = 0;
    } else if (plan.exprs[argE].retType == GX_TYPE_F64) {
      // f64 sum/avg (oracle/exec.cpp f64 path; stated-tolerance parity):
      // the value bypasses the integer VM — raw bits load through a fetch
      // slot and accumulate with f64 atomics (atomic order makes the sum
      // round differently run to run; parity tests carry the tolerance)
      const PExpr& e = plan.exprs[argE];
      int srcColF = -1;
      if (e.kind == EK_COLREF) {
        if (proj) {
          if (e.colIdx < (int)projSrcCol.size()) srcColF = projSrcCol[e.colIdx];
        } else {
          srcColF = e.colIdx;
        }
      }
      // count(f) keeps no sum: it only reads the column's NULL bitmap
      if ((ad.func != GX_AGG_SUM && ad.func != GX_AGG_AVG &&
           ad.func != GX_AGG_COUNT) || srcColF < 0) {
        ex->err = "device f64 aggregates support sum/avg over a float column";
        return GX_ERR_INVALID;
      }
      ad.fcol = srcColF;
      ad.srcReg = -1;
      ad.scale = 0;
    } else {
      const PExpr& e = plan.exprs[argE];
      if (proj) {
        if (e.kind != EK_COLREF || e.colIdx >= (int)ex->projRegs.size() ||
            ex->projRegs[e.colIdx].first < 0) {
          ex->err = "agg arg must reference a projected value";
          return GX_ERR_INVALID;
        }
        ad.srcReg = ex->projRegs[e.colIdx].first;
        ad.scale = ex->projRegs[e.colIdx].second;
      } else {
        int sc = 0;
        int reg = vmCompile(ex, ex->vm, argE, &sc);
        if (reg < 0) return GX_ERR_INVALID;
        ad.srcReg = reg;
        ad.scale = sc;
      }
    }
    ex->desc.aggs[ex->desc.nAggs++] = ad;
  }
  // physical accumulator plan: one acc slot per unique source register
  // (count/sum/avg are all additive, so aggs over the same value share)
  ex->desc.nAccSlots = 0;
  for (int a = 0; a < ex->desc.nAggs; a++) {
    const gxp::AggDesc& ad = ex->desc.aggs[a];
    if (ad.fcol >= 0 && ad.func != GX_AGG_COUNT) {
      // f64 sum/avg: slot keyed by the source column
      int found = -1;
      for (int s = 0; s < ex->desc.nAccSlots; s++)
        if (ex->desc.accKind[s] == 3 && ex->desc.accFcol[s] == ad.fcol) {
          found = s;
          break;
        }
      if (found < 0) {
        int slot = fetchSlot(ex, gxp::FETCH_8B, ad.fcol);
        if (slot < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
        found = ex->desc.nAccSlots++;
        ex->desc.accReg[found] = slot;
        ex->desc.accKind[found] = 3;
        ex->desc.accFcol[found] = ad.fcol;
      }
      ex->desc.accMap[a] = found;
      continue;
    }
    if (ad.func == GX_AGG_COUNT || ad.srcReg < 0) {
      ex->desc.accMap[a] = -1;
      continue;
    }
    // MIN stores the complemented bias so both extremes accumulate with
    // unsigned max; kind distinguishes the three accumulator behaviors
    int kind = ad.func == GX_AGG_MAX ? 1 : (ad.func == GX_AGG_MIN ? 2 : 0);
    if (kind != 0) {
      int argE2 = agg->aggArgs[a];
      if (argE2 < 0 || (plan.exprs[argE2].retType != GX_TYPE_DECIMAL &&
                        plan.exprs[argE2].retType != GX_TYPE_I64)) {
        ex->err = "device min/max supports decimal/int64 arguments this round";
        return GX_ERR_INVALID;
      }
    }
    int found = -1;
    for (int s = 0; s < ex->desc.nAccSlots; s++)
      if (ex->desc.accReg[s] == ad.srcReg && ex->desc.accKind[s] == kind) {
        found = s;
        break;
      }
    if (found < 0) {
      found = ex->desc.nAccSlots++;
      ex->desc.accReg[found] = ad.srcReg;
      ex->desc.accKind[found] = kind;
      ex->desc.accFcol[found] = -1;
    }
    ex->desc.accMap[a] = found;
  }

  // move loads to the front of the instruction stream (the kernel issues
  // [0, nLoadIns) as the batched fetch-consume pipeline), then assign their
  // raw-fetch slots in stream order
  {
    gxp::FusedQueryDesc& d = ex->desc;
    d.nLoadIns =
        finishVmProgram(ex, ex->vm, kVmLoadOps | 1u << gxp::VM_STRLEN);
    if (d.nLoadIns < 0) return GX_ERR_INVALID;
    for (int i = 0; i < d.nLoadIns; i++) {
      gxp::VmIns& ins = d.ins[i];
      ins.c = fetchSlot(ex,
                        ins.op == gxp::VM_LOAD_DEC   ? gxp::FETCH_DEC16
                        : ins.op == gxp::VM_LOAD_I64 ? gxp::FETCH_8B
                                                     : gxp::FETCH_OFFSETS,
                        ins.a);
      if (ins.c < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
    }
    d.nVmRegs = ex->vm.nextReg;  // physical register budget for kernel dispatch
    if (getenv("GX_DEBUG"))
      for (int i = 0; i < d.nIns; i++)
        fprintf(stderr, "[gx] ins[%d] op=%d dst=%d a=%d b=%d c=%d\n", i,
                d.ins[i].op, d.ins[i].dst, d.ins[i].a, d.ins[i].b, d.ins[i].c);
    // pick the fetch-pipeline depth: keep raw state within the VGPR budget
    // (~16 bytes per slot per row)
    if (d.nFetch <= 4) d.rbatch = 4;
    else d.rbatch = 2;
    if (getenv("GX_RBATCH")) d.rbatch = atoi(getenv("GX_RBATCH"));
  }
  return GX_OK;
}

// assign per-stream LDS offsets for the glds-staged kernel (64-row tiles)
static void assignGldsOffsets(gxp::FusedQueryDesc& d) {
  int off = 0;
  for (int f = 0; f < d.nFetch; f++) {
    d.fetch[f].ldsOff = off;
    int bytes = d.fetch[f].kind == gxp::FETCH_DEC16 ? 1024
                : d.fetch[f].kind == gxp::FETCH_8B ? 512
                                                   : 64;
    off += (bytes + 15) & ~15;
  }
  d.tileBytes = off;
}

// ---------------- device materialization ----------------

// upload bound host chunks into a device table (concatenated)
static int32_t uploadBoundChunks(gx_exec* ex, Binding& b, gxp::DevTable& tab) {
  int nCols = tab.nCols;
  int64_t total = 0;
  for (auto& ch : b.chunks) total += ch.empty() ? 0 : ch[0].length;
  tab.nRows = total;
  for (int c = 0; c < nCols; c++) {
    gxp::DevCol& col = tab.cols[c];
    std::vector<uint8_t> data;
    std::vector<int64_t> offsets{0};
    std::vector<uint8_t> nulls((total + 7) / 8, 0);
    int64_t row = 0;
    bool hasNulls = false;
    for (auto& ch : b.chunks) {
      const HostCol& hc = ch[c];
      for (int i = 0; i < hc.length; i++, row++) {
        bool notNull = (hc.nullBitmap[i / 8] >> (i % 8)) & 1;
        if (notNull) nulls[row / 8] |= 1 << (row % 8);
        else hasNulls = true;
      }
      if (col.type == GX_TYPE_STRING) {
        int64_t base = data.size();
        data.insert(data.end(), hc.data.begin(), hc.data.end());
        for (int i = 1; i <= hc.length; i++)
          offsets.push_back(base + hc.offsets[i]);
      } else {
        data.insert(data.end(), hc.data.begin(), hc.data.end());
      }
    }
    col.hasNulls = hasNulls ? 1 : 0;
    if (col.type == GX_TYPE_STRING) {
      bool dense = true;
      for (size_t i = 0; i < offsets.size() && dense; i++)
        if (offsets[i] != (int64_t)i) dense = false;
      col.denseOffsets = dense ? 1 : 0;
    }
    col.data = devAlloc(ex, std::max<size_t>(data.size(), 1));
    if (!col.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemcpy(col.data, data.data(), data.size(),
                         hipMemcpyHostToDevice));
    if (col.type == GX_TYPE_STRING) {
      col.offsets = (int64_t*)devAlloc(ex, offsets.size() * 8);
      if (!col.offsets) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      HIP_OK(ex, hipMemcpy(col.offsets, offsets.data(), offsets.size() * 8,
                           hipMemcpyHostToDevice));
    }
    if (hasNulls) {
      col.nullBitmap = (uint8_t*)devAlloc(ex, nulls.size());
      if (!col.nullBitmap) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      HIP_OK(ex, hipMemcpy(col.nullBitmap, nulls.data(), nulls.size(),
                           hipMemcpyHostToDevice));
    } else {
      col.nullBitmap = nullptr;
    }
  }
  return GX_OK;
}

// materialize one source (tpch generator or bound chunks) into a device table
static int32_t materializeTable(gx_exec* ex, int srcNodeId, gxp::DevTable* tab) {
  const PNode& srcNode = ex->plan.nodes[srcNodeId];
  setTableMeta(tab, srcNode.colTypes, srcNode.colFracs);
  auto it = ex->bindings.find(srcNodeId);
  if (it == ex->bindings.end()) {
    ex->err = "source not bound";
    return GX_ERR_INVALID;
  }
  Binding& b = it->second;
  if (b.haveChunks) return uploadBoundChunks(ex, b, *tab);
  if (b.tpchTable < 0) {
    ex->err = "source not bound";
    return GX_ERR_INVALID;
  }
  int64_t n = b.tpchRows;
  tab->nRows = n;
  int64_t totalRows = b.tpchTotalRows > 0 ? b.tpchTotalRows : n;
  int rc = 0;
  switch (b.tpchTable) {
    case GX_TPCH_LINEITEM: {
      for (int c = 0; c < tab->nCols; c++) {
        gxp::DevCol& col = tab->cols[c];
        if (col.type == GX_TYPE_STRING) {
          col.offsets = (int64_t*)devAlloc(ex, (n + 1) * 8);
          col.data = devAlloc(ex, std::max<int64_t>(n, 1));
          col.denseOffsets = 1;
        } else {
          col.data = devAlloc(ex, std::max<int64_t>(n * col.elemSize, 1));
        }
        if (!col.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        col.nullBitmap = nullptr;
        col.hasNulls = 0;
      }
      rc = gxp::gxLaunchTpchGen(0, tab, b.tpchRowOffset, n, b.tpchSeed,
                                totalRows, ex->stream);
      break;
    }
    case GX_TPCH_ORDERS: {
      for (int c = 0; c < 4; c++) {
        tab->cols[c].data = devAlloc(ex, std::max<int64_t>(n * 8, 1));
        if (!tab->cols[c].data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        tab->cols[c].nullBitmap = nullptr;
        tab->cols[c].hasNulls = 0;
      }
      rc = gxp::gxGenOrders(tab, b.tpchRowOffset, n, b.tpchSeed, totalRows,
                            ex->stream);
      break;
    }
    case GX_TPCH_CUSTOMER: {
      tab->cols[0].data = devAlloc(ex, std::max<int64_t>(n * 8, 1));
      tab->cols[1].offsets = (int64_t*)devAlloc(ex, (n + 1) * 8);
      if (!tab->cols[0].data || !tab->cols[1].offsets) {
        ex->err = "hipMalloc failed";
        return GX_ERR_INTERNAL;
      }
      long long totalBytes = 0;
      rc = gxp::gxGenCustomerOffsets(tab, b.tpchRowOffset, n, b.tpchSeed,
                                     ex->stream, &totalBytes);
      if (rc != 0) break;
      tab->cols[1].data = devAlloc(ex, std::max<long long>(totalBytes, 1));
      if (!tab->cols[1].data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      rc = gxp::gxGenCustomerFill(tab, b.tpchRowOffset, n, b.tpchSeed, ex->stream);
      tab->cols[0].nullBitmap = tab->cols[1].nullBitmap = nullptr;
      tab->cols[0].hasNulls = tab->cols[1].hasNulls = 0;
      tab->cols[1].denseOffsets = 0;
      break;
    }
    default:
      ex->err = "unknown synthetic table";
      return GX_ERR_INVALID;
  }
  if (rc != 0) {
    ex->err = std::string("generator failed: ") +
              hipGetErrorString((hipError_t)rc);
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  return GX_OK;
}

static int32_t finalizeFusedBind(gx_exec* ex);

static int32_t materializeDevice(gx_exec* ex) {
  if (ex->deviceReady) return GX_OK;
  if (!gpuAvailable()) {
    ex->err = "no MI355X visible: the product engine has no CPU fallback "
              "(GX_ERR_NO_GPU)";
    return GX_ERR_NO_GPU;
  }
  if (ex->device >= 0) hipSetDevice(ex->device);
  HIP_OK(ex, hipStreamCreate(&ex->stream));
  auto it = ex->bindings.find(ex->sourceNode);
  if (it == ex->bindings.end()) {
    ex->err = "source not bound";
    return GX_ERR_INVALID;
  }
  Binding& b = it->second;
  gxp::DevTable& tab = ex->desc.table;
  if (b.tpchTable >= 0 && b.tpchTable != GX_TPCH_LINEITEM) {
    // orders / customer (a general varlen column): the shared generator path
    int32_t mrc = materializeTable(ex, ex->sourceNode, &tab);
    if (mrc != GX_OK) return mrc;
  } else if (b.tpchTable >= 0) {
    tab.nRows = b.tpchRows;
    int64_t n = b.tpchRows;
    for (int c = 0; c < tab.nCols; c++) {
      gxp::DevCol& col = tab.cols[c];
      size_t bytes;
      if (col.type == GX_TYPE_STRING) {
        // generator strings are single bytes (char(1)); offsets dense
        col.offsets = (int64_t*)devAlloc(ex, (n + 1) * 8);
        col.data = devAlloc(ex, std::max<int64_t>(n, 1));
        col.denseOffsets = 1;
        if (!col.offsets || !col.data) {
          ex->err = "hipMalloc failed";
          return GX_ERR_INTERNAL;
        }
      } else {
        bytes = (size_t)n * col.elemSize;
        col.data = devAlloc(ex, std::max<size_t>(bytes, 1));
        if (!col.data) {
          ex->err = "hipMalloc failed";
          return GX_ERR_INTERNAL;
        }
      }
      col.nullBitmap = nullptr;  // synthetic data has no NULLs
      col.hasNulls = 0;
    }
    int rc = gxp::gxLaunchTpchGen(b.tpchTable, &tab, b.tpchRowOffset, n,
                                  b.tpchSeed,
                                  b.tpchTotalRows > 0 ? b.tpchTotalRows : n,
                                  ex->stream);
    if (rc != 0) {
      ex->err = "generator launch failed: " +
                std::string(hipGetErrorString((hipError_t)rc));
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
  } else if (b.haveChunks) {
    // concatenate bound chunks into one device table
    int nCols = tab.nCols;
    int64_t total = 0;
    for (auto& ch : b.chunks) total += ch.empty() ? 0 : ch[0].length;
    tab.nRows = total;
    for (int c = 0; c < nCols; c++) {
      gxp::DevCol& col = tab.cols[c];
      // host-side concat
      std::vector<uint8_t> data;
      std::vector<int64_t> offsets{0};
      std::vector<uint8_t> nulls((total + 7) / 8, 0);
      int64_t row = 0;
      bool hasNulls = false;
      for (auto& ch : b.chunks) {
        const HostCol& hc = ch[c];
        for (int i = 0; i < hc.length; i++, row++) {
          bool notNull = (hc.nullBitmap[i / 8] >> (i % 8)) & 1;
          if (notNull) nulls[row / 8] |= 1 << (row % 8);
          else hasNulls = true;
        }
        if (col.type == GX_TYPE_STRING) {
          int64_t base = data.size();
          data.insert(data.end(), hc.data.begin(), hc.data.end());
          for (int i = 1; i <= hc.length; i++)
            offsets.push_back(base + hc.offsets[i]);
        } else {  // (density of string offsets checked below)
          data.insert(data.end(), hc.data.begin(), hc.data.end());
        }
      }
      col.hasNulls = hasNulls ? 1 : 0;
      if (col.type == GX_TYPE_STRING) {
        bool dense = true;
        for (size_t i = 0; i < offsets.size() && dense; i++)
          if (offsets[i] != (int64_t)i) dense = false;
        col.denseOffsets = dense ? 1 : 0;
      }
      col.data = devAlloc(ex, std::max<size_t>(data.size(), 1));
      if (!col.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      HIP_OK(ex, hipMemcpy(col.data, data.data(), data.size(),
                           hipMemcpyHostToDevice));
      if (col.type == GX_TYPE_STRING) {
        col.offsets = (int64_t*)devAlloc(ex, offsets.size() * 8);
        if (!col.offsets) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        HIP_OK(ex, hipMemcpy(col.offsets, offsets.data(), offsets.size() * 8,
                             hipMemcpyHostToDevice));
      }
      if (hasNulls) {
        col.nullBitmap = (uint8_t*)devAlloc(ex, nulls.size());
        if (!col.nullBitmap) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        HIP_OK(ex, hipMemcpy(col.nullBitmap, nulls.data(), nulls.size(),
                             hipMemcpyHostToDevice));
      } else {
        col.nullBitmap = nullptr;
      }
    }
  } else {
    ex->err = "source not bound";
    return GX_ERR_INVALID;
  }
  return finalizeFusedBind(ex);
}

// key-record store for the serialized wide-key path (sized with the global
// table; grown together with it on kErrGlobalFull)
static int32_t ensureWideKeyStore(gx_exec* ex) {
  gxp::GroupKeyDesc& g = ex->desc.gkey;
  g.recBytes = 16 + 24 * g.nCols;
  // the record cursor doubles as the LOAD-FACTOR trigger: growth fires at
  // ~70% occupancy, long before linear probing degenerates (a near-full
  // open table costs a whole-table scan per insert)
  g.recCap = std::max<int64_t>(
      4096, ((int64_t)1 << ex->desc.globalGroupsLog2) * 7 / 10);
  g.keyStore = (uint8_t*)devAllocP(ex, (size_t)g.recCap * g.recBytes);
  if (!g.recCursor) g.recCursor = (uint64_t*)devAllocP(ex, 8);
  if (!g.keyStore || !g.recCursor) {
    ex->err = "hipMalloc failed (wide key store)";
    return GX_ERR_INTERNAL;
  }
  return GX_OK;
}

static int64_t hbmBudgetBytes();

// resident bytes of a materialized table by schema (the out-of-core
// decisions' arithmetic: 40 B decimal, 8+1 B char(1) string, 8 B otherwise)
static int64_t tableSchemaBytes(const gxp::DevTable& tab) {
  int64_t rb = 0;
  for (int c = 0; c < tab.nCols; c++) {
    int t = tab.cols[c].type;
    rb += t == GX_TYPE_DECIMAL ? 40 : (t == GX_TYPE_STRING ? 9 : 8);
  }
  return rb * tab.nRows;
}

// Second pass of a proven units column whose range fits `width` < 8 bytes
// (DESIGN.md §4i): copy it into a buffer of that width and free the int64
// one. Never an error: on any failure the column keeps its int64 buffer.
static void narrowDecUnits(gx_exec* ex, gxp::DevCol& c, int64_t nRows,
                           int width, bool dbg, int colNo) {
  void* narrow = devAllocP(ex, (size_t)gxp::unitsAllocBytes(nRows, width));
  if (!narrow) {
    (void)hipGetLastError();
    return;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (dbg) {
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, ex->stream);
  }
  bool ok = gxp::gxNarrowUnits((const int64_t*)c.units, nRows, width, narrow,
                               ex->stream) == 0;
  if (dbg) hipEventRecord(e1, ex->stream);
  ok = ok && hipStreamSynchronize(ex->stream) == hipSuccess;
  if (dbg) {
    float ms = 0;
    if (ok) hipEventElapsedTime(&ms, e0, e1);
    fprintf(stderr, "[gx] dec units col %d: width %d B%s, narrowing %.3f ms\n",
            colNo, ok ? width : 8, ok ? "" : " (narrowing failed)", ms);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  if (!ok) {
    (void)hipGetLastError();
    devFreeP(ex, narrow);
    return;
  }
  devFreeP(ex, c.units);
  c.units = narrow;
  c.unitsWidth = (uint8_t)width;
}

// Decimal units columns. `tab` is a RESIDENT source table
// (generator or bound chunks: filled once, re-read by every later open), so
// the 40 B -> int64 conversion the scan repeats per row per query is done
// here once. Each listed column gets an 8 B/row buffer filled by
// gxBuildDecUnits, then narrowed to the width its proven range needs
// (narrowDecUnits; GX_NO_UNITS_NARROW=1 keeps 8 B); a column whose proof
// fails keeps units == nullptr and its 40 B path. The budget admits the
// 8 B/row/column form; while one column is being narrowed its new buffer (at
// most 4 B/row) is live on top of that, and a failed allocation there just
// keeps the int64 buffer. Never an error: a short
// budget, a failed allocation or a failed launch all leave the query exactly
// where it was. Returns the number of columns now served from units.
static int buildDecUnits(gx_exec* ex, gxp::DevTable& tab,
                         const std::vector<int>& cols, int64_t residentBytes) {
  if (cols.empty() || tab.nRows <= 0 || getenv("GX_NO_DEC_UNITS")) return 0;
  const bool dbg = getenv("GX_DEBUG") != nullptr;
  // GX_HBM_BUDGET caps the executor's whole footprint, so the tables already
  // resident count against it; the default budget is a share of what is
  // free NOW, i.e. after materialization
  int64_t budget = hbmBudgetBytes();
  if (getenv("GX_HBM_BUDGET")) budget -= residentBytes;
  const int64_t need = (int64_t)cols.size() * tab.nRows * 8;
  if (need > budget) {
    if (dbg)
      fprintf(stderr, "[gx] dec units: %lld B over budget %lld B, not built\n",
              (long long)need, (long long)budget);
    return 0;
  }
  // per column: {proof flag, width class of the non-NULL units}
  uint32_t* flags = (uint32_t*)devAllocP(ex, cols.size() * 8);
  if (!flags) return 0;
  std::vector<int64_t*> bufs(cols.size(), nullptr);
  std::vector<hipEvent_t> evs(cols.size() + 1, nullptr);
  bool ok = hipMemsetAsync(flags, 0, cols.size() * 8, ex->stream) == hipSuccess;
  for (size_t i = 0; i < cols.size() && ok; i++) {
    bufs[i] = (int64_t*)devAllocP(ex, (size_t)tab.nRows * 8);
    ok = bufs[i] != nullptr;
  }
  if (!ok) (void)hipGetLastError();  // a failed hipMalloc is not our error
  if (ok && dbg) {
    for (auto& e : evs) hipEventCreate(&e);
    hipEventRecord(evs[0], ex->stream);
  }
  for (size_t i = 0; i < cols.size() && ok; i++) {
    const gxp::DevCol& c = tab.cols[cols[i]];
    ok = gxp::gxBuildDecUnits(c, tab.nRows, c.frac, bufs[i], flags + 2 * i,
                              ex->stream) == 0;
    if (ok && dbg) hipEventRecord(evs[i + 1], ex->stream);
  }
  std::vector<uint32_t> hflags(cols.size() * 2, 1u);
  ok = ok && hipStreamSynchronize(ex->stream) == hipSuccess &&
       hipMemcpy(hflags.data(), flags, cols.size() * 8,
                 hipMemcpyDeviceToHost) == hipSuccess;
  const bool mayNarrow = getenv("GX_NO_UNITS_NARROW") == nullptr;
  int built = 0;
  for (size_t i = 0; i < cols.size(); i++) {
    bool proven = ok && hflags[2 * i] == 0;
    if (dbg && ok) {
      float ms = 0;
      hipEventElapsedTime(&ms, evs[i], evs[i + 1]);
      fprintf(stderr, "[gx] dec units col %d frac %d: %s, build %.3f ms\n",
              cols[i], tab.cols[cols[i]].frac,
              proven ? "compacted" : "kept 40 B (proof failed)", ms);
    }
    if (proven) {
      gxp::DevCol& c = tab.cols[cols[i]];
      c.units = bufs[i];
      c.unitsWidth = 8;
      // the width class is one of 0 (no non-NULL row), 1, 2, 4, 8
      const int width = hflags[2 * i + 1] <= 1 ? 1 : (int)hflags[2 * i + 1];
      if (mayNarrow && width < 8) narrowDecUnits(ex, c, tab.nRows, width, dbg,
                                                 cols[i]);
      built++;
    } else if (bufs[i]) {
      devFreeP(ex, bufs[i]);
    }
  }
  for (auto& e : evs)
    if (e) hipEventDestroy(e);
  devFreeP(ex, flags);
  return built;
}

// bind-time fixups + result buffers for the fused aggregation, over whatever
// filled desc.table (a bound/generated source, or a materialized join
// output). Idempotent (fetch slots must not be re-assigned on re-open).
static int32_t finalizeFusedBind(gx_exec* ex) {
  if (ex->fusedBindDone) return GX_OK;
  gxp::DevTable& tab = ex->desc.table;
  // finalize group keys now that offset density is known; non-dense string
  // keys join the compile-forced reasons (decimal/time/3+ cols) in selecting
  // the serialized wide-key path
  {
    gxp::GroupKeyDesc& g = ex->desc.gkey;
    if (!g.wideMode) {
      for (int k = 0; k < g.nCols; k++)
        if (g.kind[k] == 0 && !tab.cols[g.col[k]].denseOffsets) g.wideMode = 1;
    }
    if (g.wideMode) {
      for (int k = 0; k < g.nCols; k++) {
        if (g.kind[k] == 0 || g.kind[k] == 2) {  // strings: offsets-pair fetch
          g.kind[k] = 5;
          g.slot[k] = fetchSlot(ex, gxp::FETCH_OFFSETS, g.col[k]);
          if (g.slot[k] < 0) { ex->err = "fetch plan full"; return GX_ERR_INVALID; }
        } else if (g.kind[k] == 1) {
          g.kind[k] = 3;  // raw 8B value; slot already assigned
        }
      }
      int32_t rc = ensureWideKeyStore(ex);
      if (rc) return rc;
    } else {
      for (int k = 0; k < g.nCols; k++) {
        if (g.kind[k] != 1) {
          const gxp::DevCol& c = tab.cols[g.col[k]];
          if (c.denseOffsets) {
            g.kind[k] = 2;
            g.slot[k] = fetchSlot(ex, gxp::FETCH_B1, g.col[k]);
          } else {
            g.kind[k] = 0;
            g.slot[k] = fetchSlot(ex, gxp::FETCH_OFFSETS, g.col[k]);
            if (g.slot[k] < 0) {
              ex->err = "fetch plan full";
              return GX_ERR_INVALID;
            }
          }
        }
      }
    }
  }
  // result/error buffers; low-NDV tables replicate accumulator banks to
  // spread noLds atomic contention (high-NDV tables have natural spread)
  ex->desc.accBanks = ex->desc.globalGroupsLog2 <= 16 ? 16 : 1;
  ex->devTable = (gxp::GroupSlot*)devAllocP(
      ex, (sizeof(gxp::GroupSlot) << ex->desc.globalGroupsLog2) *
              ex->desc.accBanks);
  ex->devResult =
      (gxp::FusedResultBlock*)devAllocP(ex, sizeof(gxp::FusedResultBlock));
  ex->devDesc = (gxp::FusedQueryDesc*)devAllocP(ex, sizeof(gxp::FusedQueryDesc));
  if (!ex->devTable || !ex->devResult || !ex->devDesc) {
    ex->err = "hipMalloc failed";
    return GX_ERR_INTERNAL;
  }
  // the pass's error flag and selected-row counter live in the result
  // block's header: one memset resets both, one copy brings both back
  ex->devErr = &ex->devResult->hdr.errorFlag;
  ex->devSel = &ex->devResult->hdr.selCount;
  ex->descShadow.clear();
  if (!ex->hostResult)
    HIP_OK(ex, hipHostMalloc((void**)&ex->hostResult,
                             sizeof(gxp::FusedResultBlock), hipHostMallocDefault));
  if (!ex->evK0) HIP_OK(ex, hipEventCreate(&ex->evK0));
  if (!ex->evK1) HIP_OK(ex, hipEventCreate(&ex->evK1));
  ex->desc.globalTable = ex->devTable;
  ex->desc.errorFlag = ex->devErr;
  ex->desc.selCount = ex->devSel;

  // glds-staged variant eligibility: every stream stageable, slots assigned,
  // no NULLs on any consumed column, enough rows to matter
  {
    gxp::FusedQueryDesc& d = ex->desc;
    // The glds-staged kernel is parity-green but measured slower than the
    // plain grouped-fetch kernel on Q1/SF10 (5.48 vs 4.71 ms), so it ships
    // opt-in until the pipelining wins back the staging overhead.
    bool ok = tab.nRows >= 256 && getenv("GX_GLDS") &&
              !d.gkey.wideMode &&   // wide keys use the plain kernel
              // the staged kernel's VmState is 12-reg
              ex->vm.nextReg <= kVmRegsNarrowState;
    for (int s = 0; s < d.nAccSlots && ok; s++)
      ok = d.accKind[s] == 0;  // staged accumulate is sum-only
    // the staged VM runs the core opcode set: no division, rounding or strings
    ok = ok && gxp::vmOpsWithin(d.ins, d.nIns, gxp::kVmOpsCore);
    for (int f = 0; f < d.nFetch && ok; f++)
      ok = d.fetch[f].kind == gxp::FETCH_8B ||
           d.fetch[f].kind == gxp::FETCH_DEC16 ||
           d.fetch[f].kind == gxp::FETCH_B1;
    for (int k = 0; k < d.gkey.nCols && ok; k++)
      ok = d.gkey.kind[k] != 0 && d.gkey.slot[k] >= 0;
    for (int p = 0; p < d.nPreds && ok; p++) ok = d.preds[p].slot >= 0;
    for (int c = 0; c < tab.nCols && ok; c++) ok = tab.cols[c].hasNulls == 0;
    if (ok) {
      assignGldsOffsets(d);
      d.useGlds = 1;
    } else {
      d.useGlds = 0;
    }
    // one shared row count per group when no consumed column can be NULL
    d.sharedCnt = 1;
    for (int c = 0; c < tab.nCols; c++)
      if (tab.cols[c].hasNulls) d.sharedCnt = 0;
    // plain-kernel char prefetch: when every group col is a dense char(1),
    // fold the bytes into an 8B fetch slot's unused v.y (or a standalone
    // slot) so the pipelined phase-A fetch covers the group key too -- the
    // direct per-row char load was the serial latency left in the row chain.
    for (int k = 0; k < 2; k++) d.gkey.rawSlot[k] = -1;
    if (!d.useGlds && d.gkey.nCols > 0) {
      bool allChar = true;
      for (int k = 0; k < d.gkey.nCols; k++) allChar &= d.gkey.kind[k] == 2;
      if (allChar) {
        int c0 = d.gkey.col[0];
        int c1 = d.gkey.nCols > 1 ? d.gkey.col[1] : 0;
        int packed = (c0 & 0xFF) | ((c1 & 0xFF) << 8) |
                     (d.gkey.nCols << 16);
        int slot = -1;
        for (int f = 0; f < d.nFetch; f++)
          if (d.fetch[f].kind == gxp::FETCH_8B) { slot = f; break; }
        if (slot >= 0) {
          d.fetch[slot].kind = gxp::FETCH_8B_CHAR2;
          d.fetch[slot].ldsOff = packed;
        } else if (d.nFetch < gxp::kMaxFetch) {
          slot = d.nFetch++;
          d.fetch[slot].kind = gxp::FETCH_CHAR2;
          d.fetch[slot].col = c0;
          d.fetch[slot].ldsOff = packed;
        }
        if (slot >= 0)
          for (int k = 0; k < d.gkey.nCols; k++) d.gkey.rawSlot[k] = slot;
      }
    }
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] useGlds=%d tileBytes=%d nFetch=%d\n", d.useGlds,
              d.tileBytes, d.nFetch);
  }
  // decimal units columns: the fetch plan is final, so every FETCH_DEC16
  // slot (VM loads -- decimal group keys read those registers -- and decimal
  // predicates) names a consumed decimal column. Only for a table a source
  // binding filled: streamed slices and join outputs are re-made every run
  // (the conversion would be a new pass each time), and the opt-in glds
  // variant stages the 40 B form.
  ex->decUnitsFused = 0;
  if (ex->kind != ExecKind::AGG_OVER_JOIN && !ex->fusedStreamed &&
      !ex->desc.useGlds) {
    gxp::FusedQueryDesc& d = ex->desc;
    std::vector<int> cols;
    for (int f = 0; f < d.nFetch; f++)
      if (d.fetch[f].kind == gxp::FETCH_DEC16 &&
          std::find(cols.begin(), cols.end(), d.fetch[f].col) == cols.end())
        cols.push_back(d.fetch[f].col);
    ex->decUnitsFused = buildDecUnits(ex, tab, cols, tableSchemaBytes(tab));
    // proven columns: rewrite the slot IN PLACE (slot indices never move)
    for (int f = 0; f < d.nFetch; f++)
      if (d.fetch[f].kind == gxp::FETCH_DEC16 && tab.cols[d.fetch[f].col].units)
        d.fetch[f].kind = gxp::FETCH_UNITS8;
  }
  ex->fusedBindDone = true;
  ex->deviceReady = true;
  return GX_OK;
}

// ---------------- query execution (fused path) ----------------

static void decodeGroupLane(gx_exec* ex, uint32_t lane, int kind, int type,
                            OutRowVal* v) {
  v->type = type;
  if (lane == 0xFF000000u) {
    v->isNull = true;
    return;
  }
  if (kind == 1) {
    v->i64 = (int64_t)lane;
  } else {  // kind 0 (string) and kind 2 (dense char) share the lane encoding
    int len = (int)(lane >> 24);
    v->str.clear();
    for (int j = 0; j < len; j++) v->str.push_back((char)((lane >> (8 * j)) & 0xFF));
  }
}

// a packed group key overflowed its lane (string > 3 bytes or i64 >= 2^31):
// convert every column to the serialized wide-key path. Returns false when
// the conversion is impossible (fetch plan full / key store alloc failed).
static bool convertPackedKeysToWide(gx_exec* ex) {
  gxp::GroupKeyDesc& g = ex->desc.gkey;
  bool ok = true;
  for (int k = 0; k < g.nCols && ok; k++) {
    if (g.kind[k] == 1) {
      g.kind[k] = 3;
    } else if (g.kind[k] == 0) {
      g.kind[k] = 5;  // offsets slot already assigned at bind
      ok = g.slot[k] >= 0;
    } else if (g.kind[k] == 2) {
      g.kind[k] = 5;
      g.slot[k] = fetchSlot(ex, gxp::FETCH_OFFSETS, g.col[k]);
      ok = g.slot[k] >= 0;
    }
  }
  if (!ok) return false;
  g.wideMode = 1;
  ex->desc.useGlds = 0;
  // the packed-key specializations no longer apply
  ex->jitProg = nullptr;
  ex->jitProgRepl = nullptr;
  return ensureWideKeyStore(ex) == GX_OK;
}

static int32_t fusedDecodeResults(gx_exec* ex);
static int64_t hbmBudgetBytes();

// The generated kernel for this pass, or nullptr for the interpreted one.
// Tier 0 (lane-replicated LDS accumulators) answers until a block meets more
// keys than its small table holds; each layout compiles on first use, any
// failure falls through to the next. Also records the pass's tier.
static const gxjit::JitProg* fusedPickJit(gx_exec* ex, bool mayCompile) {
  const bool dbg = getenv("GX_DEBUG") != nullptr;
  auto compile = [&](bool repl) -> const gxjit::JitProg* {
    bool eligible = !ex->desc.gkey.wideMode;  // wide keys: interpreted kernel
    for (int k = 0; k < ex->desc.gkey.nCols; k++)
      eligible &= ex->desc.gkey.kind[k] != 0;
    if (!eligible) return nullptr;
    std::string why;
    const gxjit::JitProg* p = gxjit::compile(ex->desc, repl, &why);
    if (dbg)
      fprintf(stderr, "[gx] jit %s%s%s\n", p ? "ok" : "DISABLED: ",
              p ? "" : why.c_str(), repl ? " (replicated LDS layout)" : "");
    return p;
  };
  const gxjit::JitProg* prog = nullptr;
  bool repl = false;
  if (!ex->ldsNoRepl && !ex->desc.noLds && !getenv("GX_NO_LDS_REPL")) {
    if (!ex->jitReplTried && mayCompile) {
      ex->jitReplTried = true;
      ex->jitProgRepl = compile(true);
    }
    prog = ex->jitProgRepl;
    repl = prog != nullptr;
  }
  if (!prog) {
    if (!ex->jitTried && mayCompile) {
      ex->jitTried = true;
      ex->jitProg = compile(false);
    }
    prog = ex->jitProg;
  }
  ex->lastLdsTier = ex->desc.noLds ? 2 : (repl ? 0 : 1);
  // what the pass's kernel does, not what the plan would allow: the
  // interpreted kernels take one row per lane
  ex->lastRowsPerLane = prog ? gxjit::progRowsPerLane(prog) : 1;
  return prog;
}

// reset the pass's header on the stream: error flag and group cursor always,
// the selected-row count unless a later streaming slice keeps counting
static hipError_t fusedResetHeader(gx_exec* ex, bool keepSel) {
  return hipMemsetAsync(&ex->devResult->hdr, 0,
                        keepSel ? offsetof(gxp::FusedResultHdr, selCount)
                                : sizeof(gxp::FusedResultHdr),
                        ex->stream);
}

// upload the descriptor only when it differs from the last uploaded copy
// (a retry that edits the descriptor uploads naturally)
static hipError_t fusedUploadDesc(gx_exec* ex) {
  const size_t n = sizeof(ex->desc);
  if (ex->descShadow.size() == n &&
      std::memcmp(ex->descShadow.data(), &ex->desc, n) == 0)
    return hipSuccess;
  ex->descShadow.resize(n);
  std::memcpy(ex->descShadow.data(), &ex->desc, n);
  return hipMemcpyAsync(ex->devDesc, ex->descShadow.data(), n,
                        hipMemcpyHostToDevice, ex->stream);
}

// end of a pass: with `groups`, compact the occupied slots into the result
// block (wide-key plans keep the full-table download: the decode needs their
// key records), then ONE copy of header (+ records) into the pinned block and
// ONE sync. Every retry branch reads the flag from that header.
static int32_t fusedFetchResult(gx_exec* ex, bool groups) {
  size_t bytes = sizeof(gxp::FusedResultHdr);
  ex->resultCompact = false;
  if (groups && !ex->desc.gkey.wideMode) {
    int lrc = gxp::gxLaunchCompactGroups(
        ex->devDesc, ex->desc.globalGroupsLog2,
        ex->desc.noLds ? ex->desc.accBanks : 1, ex->devResult, ex->stream);
    if (lrc != 0) {
      ex->err = "group compaction launch failed: " +
                std::string(hipGetErrorString((hipError_t)lrc));
      return GX_ERR_INTERNAL;
    }
    bytes = sizeof(gxp::FusedResultBlock);
    ex->resultCompact = true;
  }
  HIP_OK(ex, hipMemcpyAsync(ex->hostResult, ex->devResult, bytes,
                            hipMemcpyDeviceToHost, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  return GX_OK;
}

// out-of-core aggregation (the agg_spill.go analog, MI355X-shaped): the
// GROUP STATES stay resident in HBM — bounded by the grown global table —
// while INPUT row-range slices stream through the fused kernel, every slice
// accumulating into the SAME table (skipInit). Retryable device flags
// (narrow overflow, LDS/global-table growth, packed-key overflow) restart
// the whole slice loop with the new setting, exactly like the one-shot path.
static int32_t runFusedStreaming(gx_exec* ex, Binding& b, int64_t sliceRows) {
  const int64_t total = b.tpchRows, saveOff = b.tpchRowOffset;
  const int64_t saveTot = b.tpchTotalRows > 0 ? b.tpchTotalRows : total;
  ex->fusedStreamed = true;
  int32_t rc = GX_OK;
  if (getenv("GX_DEBUG"))
    fprintf(stderr, "[gx] fused agg streaming: %lld rows in %lld-row slices\n",
            (long long)total, (long long)sliceRows);
restart:
  ex->lastKernelMs = 0;
  for (int64_t done = 0; done < total;) {
    int64_t n = std::min(sliceRows, total - done);
    size_t mark = ex->devBufs.size();
    b.tpchRows = n;
    b.tpchRowOffset = saveOff + done;
    b.tpchTotalRows = saveTot;
    ex->deviceReady = false;
    rc = materializeDevice(ex);
    if (rc) goto out;
    if (done == 0) {
      // string group keys through the wide path verify/decode via OWNER ROW
      // references into the source table — slices are freed, so those
      // references would dangle. Fail loudly (decimal/int/time wide keys and
      // all packed keys stream fine).
      for (int k = 0; k < ex->desc.gkey.nCols; k++)
        if (ex->desc.gkey.wideMode && ex->desc.gkey.kind[k] == 5) {
          ex->err = "string group keys over out-of-core inputs unsupported "
                    "this round";
          rc = GX_ERR_INVALID;
          goto out;
        }
    }
    {
      ex->desc.ablate = 0;
      HIP_OK(ex, fusedResetHeader(ex, done != 0));
      HIP_OK(ex, fusedUploadDesc(ex));
      if (ex->desc.noLds) ex->desc.useGlds = 0;
      HIP_OK(ex, hipEventRecord(ex->evK0, ex->stream));
      const gxjit::JitProg* prog =
          fusedPickJit(ex, !ex->desc.useGlds && !getenv("GX_NO_JIT"));
      int lrc;
      if (prog) {
        lrc = done == 0 ? gxp::gxLaunchInitTable(
                              ex->desc.globalTable,
                              (int64_t)(1 << ex->desc.globalGroupsLog2) *
                                  (ex->desc.noLds ? ex->desc.accBanks : 1),
                              ex->stream)
                        : 0;
        if (lrc == 0 && done == 0 && ex->desc.gkey.wideMode &&
            ex->desc.gkey.recCursor)
          lrc = (int)hipMemsetAsync(ex->desc.gkey.recCursor, 0, 8, ex->stream);
        if (lrc == 0)
          lrc = gxjit::launch(prog, ex->desc.wide != 0, ex->devDesc,
                              gxp::gxFusedGrid(ex->desc.table.nRows),
                              ex->stream);
      } else {
        lrc = gxp::gxLaunchFusedAgg(ex->desc, ex->devDesc, ex->stream,
                                    done != 0);
      }
      if (lrc != 0) {
        ex->err = "fused kernel launch failed: " +
                  std::string(hipGetErrorString((hipError_t)lrc));
        rc = GX_ERR_INTERNAL;
        goto out;
      }
      HIP_OK(ex, hipEventRecord(ex->evK1, ex->stream));
      // the last slice also compacts the groups: the table is complete then
      rc = fusedFetchResult(ex, done + n >= total);
      if (rc) goto out;
      float ms = 0;
      hipEventElapsedTime(&ms, ex->evK0, ex->evK1);
      ex->lastKernelMs += ms;
    }
    uint32_t errFlag = ex->hostResult->hdr.errorFlag;
    if ((errFlag & 64u) && !ex->ldsNoRepl) {
      ex->ldsNoRepl = true;
      freeSince(ex, mark);
      goto restart;
    }
    if (errFlag == 256u && !ex->desc.wide) {
      ex->desc.wide = 1;
      freeSince(ex, mark);
      goto restart;
    }
    if ((errFlag & 16u) && !ex->desc.noLds) {
      ex->desc.noLds = 1;
      freeSince(ex, mark);
      goto restart;
    }
    if ((errFlag & 32u) && ex->desc.globalGroupsLog2 < 27) {
      ex->desc.globalGroupsLog2 += 3;
      devFreeP(ex, ex->devTable);
      ex->desc.accBanks = ex->desc.globalGroupsLog2 <= 16 ? 16 : 1;
      ex->desc.globalTable = ex->devTable = (gxp::GroupSlot*)devAllocP(
          ex, (sizeof(gxp::GroupSlot) << ex->desc.globalGroupsLog2) *
                  ex->desc.accBanks);
      if (!ex->devTable) {
        ex->err = "hipMalloc failed (group table)";
        rc = GX_ERR_INTERNAL;
        goto out;
      }
      if (ex->desc.gkey.wideMode) {
        devFreeP(ex, ex->desc.gkey.keyStore);
        rc = ensureWideKeyStore(ex);
        if (rc) goto out;
      }
      freeSince(ex, mark);
      goto restart;
    }
    if ((errFlag & 2u) && !ex->desc.gkey.wideMode && ex->desc.gkey.nCols > 0 &&
        convertPackedKeysToWide(ex)) {
      freeSince(ex, mark);
      goto restart;
    }
    errFlag &= ~256u;
    if (errFlag != 0) {
      ex->err = "device execution error flag 0x" + std::to_string(errFlag) +
                " (unsupported data shape or overflow)";
      rc = GX_ERR_INTERNAL;
      goto out;
    }
    freeSince(ex, mark);
    done += n;
  }
out:
  b.tpchRows = total;
  b.tpchRowOffset = saveOff;
  b.tpchTotalRows = saveTot;
  if (rc) return rc;
  ex->lastSelCount = ex->hostResult->hdr.selCount;
  return fusedDecodeResults(ex);
}

static int32_t runFused(gx_exec* ex) {
  if (ex->vm.hasDiv && !getenv("GX_DIV_NARROW"))
    ex->desc.wide = 1;  // DIV quotients rarely fit int64
  ex->desc.hasDiv = ex->vm.hasDiv ? 1 : 0;
  ex->desc.nVmRegs = ex->vm.nextReg;
  if (getenv("GX_FORCE_WIDE")) ex->desc.wide = 1;
  // out-of-core aggregation: a generator source above the HBM budget
  // streams in row-range slices instead of materializing whole
  if ((!ex->deviceReady || ex->fusedStreamed) &&
      ex->kind != ExecKind::AGG_OVER_JOIN && ex->sourceNode >= 0) {
    auto itb = ex->bindings.find(ex->sourceNode);
    if (itb != ex->bindings.end() && !itb->second.haveChunks &&
        itb->second.tpchTable >= 0) {
      int64_t rb = 0;
      for (int c = 0; c < ex->desc.table.nCols; c++) {
        int t = ex->desc.table.cols[c].type;
        rb += t == GX_TYPE_DECIMAL ? 40 : (t == GX_TYPE_STRING ? 9 : 8);
      }
      int64_t need = itb->second.tpchRows * rb;
      int64_t budget = hbmBudgetBytes();
      if (ex->fusedStreamed || need > budget) {
        int64_t sliceRows = std::max<int64_t>(
            4096, budget / 2 / std::max<int64_t>(rb, 1));
        return runFusedStreaming(ex, itb->second, sliceRows);
      }
    }
  }
  int32_t rc = materializeDevice(ex);
  if (rc) return rc;
  ex->split.begin();
  ex->desc.ablate = getenv("GX_ABLATE") ? atoi(getenv("GX_ABLATE")) : 0;
  HIP_OK(ex, fusedResetHeader(ex, false));
  HIP_OK(ex, fusedUploadDesc(ex));
  HIP_OK(ex, hipEventRecord(ex->evK0, ex->stream));
  ex->split.lap(0);
  if (ex->desc.noLds) ex->desc.useGlds = 0;  // high-NDV retry uses the plain kernel
  // runtime kernel specialization (gx_jit.cpp): each layout compiles once
  // per executor, any failure -> interpreted path. Disabled for the glds
  // variant, timing ablations and general string group keys.
  const gxjit::JitProg* prog = fusedPickJit(
      ex, !ex->desc.useGlds && ex->desc.ablate == 0 && !getenv("GX_NO_JIT"));
  if (getenv("GX_DEBUG_DESC")) {
    fprintf(stderr, "[host] sizeof(desc)=%d aggs_off=%d ins_off=%d\n",
            (int)sizeof(gxp::FusedQueryDesc),
            (int)((char*)&ex->desc.aggs[0] - (char*)&ex->desc),
            (int)((char*)&ex->desc.ins[0] - (char*)&ex->desc));
    gxp::gxDumpDesc(ex->devDesc, ex->stream);
  }
  int lrc;
  if (prog) {
    lrc = gxp::gxLaunchInitTable(
        ex->desc.globalTable,
        (int64_t)(1 << ex->desc.globalGroupsLog2) *
            (ex->desc.noLds ? ex->desc.accBanks : 1),
        ex->stream);
    if (lrc == 0)
      lrc = gxjit::launch(prog, ex->desc.wide != 0, ex->devDesc,
                          gxp::gxFusedGrid(ex->desc.table.nRows), ex->stream);
  } else {
    lrc = gxp::gxLaunchFusedAgg(ex->desc, ex->devDesc, ex->stream);
  }
  if (lrc != 0) {
    ex->err = "fused kernel launch failed: " +
              std::string(hipGetErrorString((hipError_t)lrc));
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipEventRecord(ex->evK1, ex->stream));
  ex->split.lap(1);
  rc = fusedFetchResult(ex, true);
  if (rc) return rc;
  {
    float ms = 0;
    hipEventElapsedTime(&ms, ex->evK0, ex->evK1);
    ex->lastKernelMs = ms;
  }
  ex->split.lap(2);
  uint32_t errFlag = ex->hostResult->hdr.errorFlag;
  if ((errFlag & 64u /*kErrLdsSmall*/) && !ex->ldsNoRepl) {
    // a block met more keys than the replicated LDS table holds: rerun with
    // the 64-slot single-copy layout (sticky for this executor; the block-
    // entry flag check made the doomed pass cheap)
    ex->ldsNoRepl = true;
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] replicated LDS table full -> single-copy retry\n");
    return runFused(ex);
  }
  if (errFlag == 256u /*kErrRetryWide only*/ && !ex->desc.wide) {
    // a value overflowed the int64 fast path: rerun with the int128 VM
    // (sticky for this executor)
    ex->desc.wide = 1;
    if (getenv("GX_DEBUG")) fprintf(stderr, "[gx] narrow overflow -> wide retry\n");
    return runFused(ex);
  }
  if ((errFlag & 16u /*kErrLdsFull*/) && !ex->desc.noLds) {
    // more groups than the LDS table holds: rerun aggregating directly into
    // the global table (the init kernel resets it, so the rerun is clean)
    ex->desc.noLds = 1;
    if (getenv("GX_DEBUG")) fprintf(stderr, "[gx] LDS table full -> global-direct retry\n");
    return runFused(ex);
  }
  if ((errFlag & 32u /*kErrGlobalFull*/) && ex->desc.globalGroupsLog2 < 27) {
    // NDV above the global table: rerun with an 8x table (capped 2^27 groups
    // ~ 10 GB of state; the init kernel resets it, so the rerun is clean)
    ex->desc.globalGroupsLog2 += 3;
    devFreeP(ex, ex->devTable);  // the outgrown table is dead weight
    ex->desc.accBanks = ex->desc.globalGroupsLog2 <= 16 ? 16 : 1;
    ex->desc.globalTable = ex->devTable = (gxp::GroupSlot*)devAllocP(
        ex, (sizeof(gxp::GroupSlot) << ex->desc.globalGroupsLog2) *
                ex->desc.accBanks);
    if (!ex->devTable) { ex->err = "hipMalloc failed (group table)"; return GX_ERR_INTERNAL; }
    if (ex->desc.gkey.wideMode) {  // key-record store grows with the table
      devFreeP(ex, ex->desc.gkey.keyStore);
      int32_t rc2 = ensureWideKeyStore(ex);
      if (rc2) return rc2;
    }
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] global table full -> 2^%d retry\n",
              ex->desc.globalGroupsLog2);
    return runFused(ex);
  }
  if ((errFlag & 2u /*kErrBadKey*/) && !ex->desc.gkey.wideMode &&
      ex->desc.gkey.nCols > 0 && convertPackedKeysToWide(ex)) {
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] packed key overflow -> wide-key retry\n");
    return runFused(ex);
  }
  errFlag &= ~256u;
  if (ex->desc.ablate != 0 && getenv("GX_DEBUG"))
    fprintf(stderr, "[gx] ABLATE=%d kms=%.3f\n", ex->desc.ablate, ex->lastKernelMs);
  if (errFlag != 0) {
    ex->err = "device execution error flag 0x" + std::to_string(errFlag) +
              " (unsupported data shape or overflow)";
    return GX_ERR_INTERNAL;
  }
  ex->lastSelCount = ex->hostResult->hdr.selCount;
  if (getenv("GX_DEBUG")) {
    fprintf(stderr,
            "[gx] nRows=%lld nPreds=%d nIns=%d nAggs=%d gkeyCols=%d sel=%llu "
            "kms=%.3f lds_tier=%d (0 replicated x%d slots, 1 single, 2 global)\n",
            (long long)ex->desc.table.nRows, ex->desc.nPreds, ex->desc.nIns,
            ex->desc.nAggs, ex->desc.gkey.nCols,
            (unsigned long long)ex->lastSelCount, ex->lastKernelMs,
            ex->lastLdsTier, gxjit::replSlots(ex->desc));
  }
  return fusedDecodeResults(ex);
}

// occupied group slots of the last fused pass, in key order: the compact
// block when it answers, else the whole table (it lands in *table)
static int32_t collectGroupSlots(gx_exec* ex, std::vector<gxp::GroupSlot>* table,
                                 std::vector<const gxp::GroupSlot*>* occ) {
  const int64_t nSlots1 = (int64_t)1 << ex->desc.globalGroupsLog2;
  // banks beyond 0 are written ONLY by the AOT noLds direct-accumulate
  // path; the LDS flush and the hipRTC kernels land in bank 0 — download
  // and fold just bank 0 otherwise (a 16x table D2H every step cost the
  // Q1 decode ~28 ms of pure host overhead)
  const int usedBanks = ex->desc.noLds ? ex->desc.accBanks : 1;
  // the compact block answers unless it overflowed or the pass skipped it
  // (wide keys); then the whole table comes down as before
  const bool compact =
      ex->resultCompact && gxp::collectCompactGroups(*ex->hostResult, occ);
  ex->lastDecodeCompact = compact;
  if (!compact) {
    occ->clear();
    table->resize((size_t)nSlots1 * usedBanks);
    HIP_OK(ex, hipMemcpy(table->data(), ex->devTable,
                         table->size() * sizeof(gxp::GroupSlot),
                         hipMemcpyDeviceToHost));
    // fold the accumulator banks into bank 0 (gxp::foldGroupSlot, the fold
    // compactGroupsKernel applies on device)
    const int nCnt = ex->desc.sharedCnt ? 1 : ex->desc.nAggs;
    for (int bank = 1; bank < usedBanks; bank++)
      for (int64_t i = 0; i < nSlots1; i++)
        if ((*table)[i].key != gxp::kEmptyKey)
          gxp::foldGroupSlot((*table)[i], (*table)[bank * nSlots1 + i],
                             ex->desc.nAccSlots, ex->desc.accKind, nCnt);
    table->resize((size_t)nSlots1);
    for (auto& s : *table)
      if (s.key != gxp::kEmptyKey) occ->push_back(&s);
  }
  ex->split.lap(5);
  // occupied slots in deterministic order (by key)
  std::sort(occ->begin(), occ->end(),
            [](const gxp::GroupSlot* a, const gxp::GroupSlot* b) {
              return a->key < b->key;
            });
  if (getenv("GX_DEBUG"))
    fprintf(stderr, "[gx] occupied group slots: %zu\n", occ->size());
  return GX_OK;
}

// group column k of one wide-key record -> value, plus its canonical bytes
static int32_t decodeWideCol(gx_exec* ex, const std::vector<uint8_t>& recs,
                             uint64_t nRecs, const gxp::GroupSlot* s, int k,
                             OutRowVal* v, std::string* canon) {
  const gxp::GroupKeyDesc& g = ex->desc.gkey;
  uint32_t recIdx = (uint32_t)(s->key & 0xFFFFFFFFu);
  if ((uint64_t)recIdx >= nRecs) {
    ex->err = "wide key record index out of range";
    return GX_ERR_INTERNAL;
  }
  const uint8_t* rec = recs.data() + (size_t)recIdx * g.recBytes;
  const uint64_t* r64 = (const uint64_t*)rec;
  int srcCol = g.col[k];
  if (srcCol >= 0) v->type = ex->desc.table.cols[srcCol].type;
  else v->type = srcCol == -2 ? GX_TYPE_I64 : GX_TYPE_DECIMAL;
  if ((r64[0] >> k) & 1) {
    v->isNull = true;
    canon->push_back('\x01');
    return GX_OK;
  }
  canon->push_back('\x02');
  const uint64_t* f = (const uint64_t*)(rec + 16 + 24 * k);
  if (g.kind[k] == 3) {
    v->i64 = (int64_t)f[0];
    v->u64 = f[0];
    canon->append((const char*)&f[0], 8);
  } else if (g.kind[k] == 4) {
    __int128 units = ((__int128)(int64_t)f[1] << 64) | f[0];
    if (g.col[k] == -2) {  // computed i64 key (e.g. YEAR(t))
      v->type = GX_TYPE_I64;
      v->i64 = (int64_t)units;
      v->u64 = (uint64_t)v->i64;
    } else {
      v->type = GX_TYPE_DECIMAL;
      v->dec = decFromUnits(units, g.kscale[k]);
    }
    canon->append((const char*)&f[0], 16);
  } else {  // kind 5: trimmed string (prefix inline, tail via owner row)
    uint64_t len = f[0];
    v->type = GX_TYPE_STRING;
    v->str.clear();
    const char* pfx = (const char*)&f[1];
    for (uint64_t j = 0; j < len && j < 16; j++) v->str.push_back(pfx[j]);
    if (len > 16) {
      int64_t owner = (int64_t)r64[1];
      const gxp::DevCol& c = ex->desc.table.cols[srcCol];
      int64_t os = 0;
      HIP_OK(ex, hipMemcpy(&os, c.offsets + owner, 8, hipMemcpyDeviceToHost));
      std::vector<uint8_t> tail((size_t)len - 16);
      HIP_OK(ex, hipMemcpy(tail.data(), (const uint8_t*)c.data + os + 16,
                           tail.size(), hipMemcpyDeviceToHost));
      v->str.append((const char*)tail.data(), tail.size());
    }
    canon->append((const char*)&len, 8);
    canon->append(v->str);
  }
  return GX_OK;
}

// wide-key mode: download the key records and decode each occupied slot's
// group values; slot keys pack (hash32|recordIdx), so deterministic output
// order comes from sorting by the DECODED canonical values instead
static int32_t decodeWideKeys(gx_exec* ex,
                              std::vector<const gxp::GroupSlot*>* occ,
                              std::map<const gxp::GroupSlot*, ResultRow>* vals) {
  const gxp::GroupKeyDesc& g = ex->desc.gkey;
  uint64_t nRecs = 0;
  HIP_OK(ex, hipMemcpy(&nRecs, g.recCursor, 8, hipMemcpyDeviceToHost));
  if (nRecs > (uint64_t)g.recCap) nRecs = (uint64_t)g.recCap;
  std::vector<uint8_t> recs((size_t)nRecs * g.recBytes);
  if (nRecs)
    HIP_OK(ex, hipMemcpy(recs.data(), g.keyStore, recs.size(),
                         hipMemcpyDeviceToHost));
  std::map<const gxp::GroupSlot*, std::string> canonOf;
  for (const gxp::GroupSlot* s : *occ) {
    ResultRow row(g.nCols);
    std::string ck;
    for (int k = 0; k < g.nCols; k++) {
      int32_t rc = decodeWideCol(ex, recs, nRecs, s, k, &row[k], &ck);
      if (rc) return rc;
    }
    canonOf[s] = std::move(ck);
    (*vals)[s] = std::move(row);
  }
  std::sort(occ->begin(), occ->end(),
            [&](const gxp::GroupSlot* a, const gxp::GroupSlot* b) {
              return canonOf[a] < canonOf[b];
            });
  return GX_OK;
}

// group column k of a slot: the decoded wide record, else the packed lane
static OutRowVal groupKeyVal(gx_exec* ex, const gxp::GroupSlot* s, int k,
                             const ResultRow* wide) {
  if (wide) return (*wide)[k];
  OutRowVal v;
  int srcCol = ex->desc.gkey.col[k];
  decodeGroupLane(ex, (uint32_t)(s->key >> (32 * k)), ex->desc.gkey.kind[k],
                  ex->desc.table.cols[srcCol].type, &v);
  return v;
}

// one group slot -> one result row (group keys, then every aggregate's
// final value; PARTIAL mode emits the canonical (state, count) pairs)
static int32_t slotToRow(gx_exec* ex, const gxp::GroupSlot* s,
                         const ResultRow* wide, ResultRow* row) {
  const PNode& agg = ex->plan.nodes[ex->aggRoot];
  const bool partial = agg.aggMode == GX_AGG_MODE_PARTIAL;
  for (int k = 0; k < ex->desc.gkey.nCols; k++)
    row->push_back(groupKeyVal(ex, s, k, wide));
  for (int a = 0; a < ex->desc.nAggs; a++) {
    const gxp::AggDesc& ad = ex->desc.aggs[a];
    int phys = ex->desc.accMap[a];
    __int128 acc = phys >= 0
        ? (((__int128)s->accHi[phys] << 64) | s->accLo[phys]) : 0;
    int64_t cnt = s->cnt[ex->desc.sharedCnt ? 0 : a];
    if (getenv("GX_DEBUG_DESC") && phys >= 0)
      fprintf(stderr, "[host] agg%d acc lo=%llu hi=%lld cnt=%lld\n", (int)a,
              (unsigned long long)s->accLo[phys], (long long)s->accHi[phys],
              (long long)cnt);
    OutRowVal v;
    bool withCount = false;  // a PARTIAL SUM/AVG state is (sum, count)
    if (ad.fr >= 0) {  // firstrow(group col): decode from the group key
      v = groupKeyVal(ex, s, ad.fr, wide);
    } else if (ad.func == GX_AGG_COUNT) {
      v.type = GX_TYPE_I64;
      v.i64 = cnt;
    } else if (phys >= 0 && ex->desc.accKind[phys] == 3) {  // f64 sum/avg
      double sum;
      std::memcpy(&sum, &s->accLo[phys], 8);
      gxp::finalizeF64Agg(partial ? GX_AGG_SUM : ad.func, sum, cnt, &v);
      withCount = partial;
    } else if (ad.func == GX_AGG_MIN || ad.func == GX_AGG_MAX) {
      // biased-u64 extreme (accKind 1/2); NULL when no non-null arg row
      uint64_t raw = s->accLo[phys];
      if (ex->desc.accKind[phys] == 2) raw = ~raw;
      int64_t ext = (int64_t)(raw ^ 0x8000000000000000ULL);
      // output type follows the argument's type (func_max_min.go keeps the
      // arg type)
      int argE = agg.aggArgs[a];
      int srcType = argE >= 0 ? ex->plan.exprs[argE].retType
                              : GX_TYPE_DECIMAL;
      v.type = srcType;
      if (cnt == 0) {
        v.isNull = true;
      } else if (srcType == GX_TYPE_I64) {
        v.i64 = ext;
      } else {
        v.type = GX_TYPE_DECIMAL;
        v.dec = decFromUnits((__int128)ext, ad.scale);
      }
    } else if (partial) {
      v.type = GX_TYPE_DECIMAL;
      if (ad.func == GX_AGG_SUM && cnt == 0) v.isNull = true;
      else v.dec = decFromUnits(acc, ad.scale);
      withCount = true;
    } else if (!gxp::finalizeDecimalAgg(ad.func, decFromUnits(acc, ad.scale),
                                        cnt, agg.aggFracs[a], &v)) {
      ex->err = "avg finalize failed";
      return GX_ERR_INTERNAL;
    }
    row->push_back(std::move(v));
    if (withCount) {
      row->emplace_back();  // an I64 cell
      row->back().i64 = cnt;
    }
  }
  return GX_OK;
}

// download the group states and decode the result rows (shared by the
// one-shot and the out-of-core streaming paths)
static int32_t fusedDecodeResults(gx_exec* ex) {
  std::vector<gxp::GroupSlot> table;
  std::vector<const gxp::GroupSlot*> occ;
  int32_t rc = collectGroupSlots(ex, &table, &occ);
  if (rc) return rc;
  std::map<const gxp::GroupSlot*, ResultRow> wideVals;
  if (ex->desc.gkey.wideMode != 0) {
    rc = decodeWideKeys(ex, &occ, &wideVals);
    if (rc) return rc;
  }
  const PNode& agg = ex->plan.nodes[ex->aggRoot];
  ex->resultRows.clear();
  // zero-row, no-group-by => one row (count=0, sums NULL); occ points at
  // `zero`, so it is declared here to outlive the loop below
  gxp::GroupSlot zero{};
  if (occ.empty() && agg.exprs.empty() &&
      agg.aggMode != GX_AGG_MODE_PARTIAL)
    occ.push_back(&zero);
  for (const gxp::GroupSlot* s : occ) {
    auto w = wideVals.find(s);
    ResultRow row;
    rc = slotToRow(ex, s, w == wideVals.end() ? nullptr : &w->second, &row);
    if (rc) return rc;
    ex->resultRows.push_back(std::move(row));
  }
  ex->split.lap(6);
  ex->split.print();
  if (ex->distinct.nKeys >= 0) {
    rc = gxp::foldDistinct(&ex->resultRows, ex->distinct, &ex->err);
    if (rc) return rc;
  }
  if (!ex->having.empty()) {
    // HAVING over the decoded group rows (host; O(#groups))
    std::vector<ResultRow> kept;
    kept.reserve(ex->resultRows.size());
    for (ResultRow& r : ex->resultRows) {
      bool typeOk = true;
      bool pass = gxp::havingPass(r, ex->having, &typeOk);
      if (!typeOk) {
        ex->err = kHavingErr;
        return GX_ERR_INVALID;
      }
      if (pass) kept.push_back(std::move(r));
    }
    ex->resultRows = std::move(kept);
  }
  if (ex->postSort)
    gxp::sortAndSlice(&ex->resultRows, ex->postSortKeys, ex->postOffset,
                      ex->postLimit);
  return GX_OK;
}

// ---------------- join-aggregate execution (Q3 class) ----------------

static int ceilLog2(uint64_t v) {
  int l = 0;
  while ((1ULL << l) < v) l++;
  return l;
}

static int32_t runJoinAgg(gx_exec* ex) {
  gxp::JoinAggDesc& ja = ex->ja;
  if (!ex->deviceReady) {
    if (!gpuAvailable()) {
      ex->err = "no MI355X visible: the product engine has no CPU fallback "
                "(GX_ERR_NO_GPU)";
      return GX_ERR_NO_GPU;
    }
    if (ex->device >= 0) hipSetDevice(ex->device);
    HIP_OK(ex, hipStreamCreate(&ex->stream));
    int32_t rc = materializeTable(ex, ex->jaSrcCust, &ja.build0);
    if (rc) return rc;
    rc = materializeTable(ex, ex->jaSrcOrd, &ja.build1);
    if (rc) return rc;
    // the group slots carry payload values without a NULL flag: a NULL
    // payload would come back as whatever bytes lie under it. A comparison
    // conjunct on the column rejects its NULL rows before they reach a slot
    // (evalSimplePred; these filters are plain conjunctions); IS NULL keeps
    // them.
    auto nullsFiltered = [&](int col) {
      auto covers = [&](const gxp::PredDesc& p) {
        return p.col == col &&
               !(p.kind == gxp::PRED_IS_NULL && p.cmp == 4 /*GX_F_EQ*/);
      };
      if (ja.nPred1 > 0 && covers(ja.pred1)) return true;
      for (int i = 0; i < ja.nPred1x; i++)
        if (covers(ja.pred1x[i])) return true;
      return false;
    };
    for (int pc : {ja.payloadCol0, ja.payloadCol1})
      if (pc >= 0 && ja.build1.cols[pc].hasNulls && !nullsFiltered(pc)) {
        ex->err = "nullable build payload column unsupported in the "
                  "join-aggregate pipeline";
        return GX_ERR_INVALID;
      }
    rc = materializeTable(ex, ex->jaSrcLi, &ja.probe);
    if (rc) return rc;
    ex->devErr = (uint32_t*)devAllocP(ex, 4);
    ja.counters = (uint64_t*)devAllocP(ex, 3 * 8);
    ex->devJa = (gxp::JoinAggDesc*)devAllocP(ex, sizeof(gxp::JoinAggDesc));
    if (!ex->devErr || !ja.counters || !ex->devJa) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
    ja.errorFlag = ex->devErr;
    // the probe table is resident across opens: serve the decimal columns
    // its value VM loads from units columns (the build tables carry no
    // decimals on this path)
    {
      std::vector<int> cols;
      for (int i = 0; i < ja.nIns; i++)
        if (ja.ins[i].op == gxp::VM_LOAD_DEC &&
            std::find(cols.begin(), cols.end(), ja.ins[i].a) == cols.end())
          cols.push_back(ja.ins[i].a);
      ex->decUnitsJa = buildDecUnits(
          ex, ja.probe, cols,
          tableSchemaBytes(ja.build0) + tableSchemaBytes(ja.build1) +
              tableSchemaBytes(ja.probe));
    }
    ex->deviceReady = true;
  }
  HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
  HIP_OK(ex, hipMemsetAsync(ja.counters, 0, 24, ex->stream));

  auto pushDesc = [&]() -> int32_t {
    HIP_OK(ex, hipMemcpyAsync(ex->devJa, &ja, sizeof(ja),
                              hipMemcpyHostToDevice, ex->stream));
    return GX_OK;
  };
  auto phase = [&](int ph) -> int32_t {
    if (ph <= 3 && ex->jaBuildProg) {
      int64_t rows = (ph <= 1 ? ja.build0 : ja.build1).nRows;
      int jrc = gxjit::launchJaBuild(ex->jaBuildProg, ph, ex->devJa,
                                     gxp::gxFusedGrid(rows), ex->stream);
      if (jrc != 0) {
        ex->err = std::string("jit build launch failed: ") +
                  hipGetErrorString((hipError_t)jrc);
        return GX_ERR_INTERNAL;
      }
      return GX_OK;
    }
    if (ph == 4 && ex->jaJitProg) {
      int jrc = gxjit::launchJa(ex->jaJitProg, ja.wide != 0, ex->devJa,
                                gxp::gxFusedGrid(ja.probe.nRows), ex->stream);
      if (jrc != 0) {
        ex->err = std::string("jit probe launch failed: ") +
                  hipGetErrorString((hipError_t)jrc);
        return GX_ERR_INTERNAL;
      }
      return GX_OK;
    }
    int rc = gxp::gxJoinAggPhase(ph, ex->devJa, ja, ex->stream);
    if (rc != 0) {
      ex->err = std::string("join phase launch failed: ") +
                hipGetErrorString((hipError_t)rc);
      return GX_ERR_INTERNAL;
    }
    return GX_OK;
  };
  auto readCounter = [&](int i, uint64_t* out) -> int32_t {
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    HIP_OK(ex, hipMemcpy(out, ja.counters + i, 8, hipMemcpyDeviceToHost));
    return GX_OK;
  };

  // specialize the build kernels once per executor (gx_jit.cpp)
  if (!ex->jaBuildTried && !getenv("GX_NO_JIT")) {
    ex->jaBuildTried = true;
    std::string why;
    ex->jaBuildProg = gxjit::compileJaBuild(ja, &why);
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] ja build jit %s%s\n",
              ex->jaBuildProg ? "ok" : "DISABLED: ",
              ex->jaBuildProg ? "" : why.c_str());
  }

  // build0: count, size the key set, fill
  int32_t rc = pushDesc();
  if (rc) return rc;
  if ((rc = phase(0))) return rc;
  uint64_t n0 = 0;
  if ((rc = readCounter(0, &n0))) return rc;
  int wantLog2 = ceilLog2(std::max<uint64_t>(2 * n0 + 1, 64));
  // bloom over the build0 key set: rejects ~80% of build1 rows before the
  // key-set random access (Q3: 3M BUILDING customers vs 15M custkeys)
  {
    int b0Log2 = ceilLog2(std::max<uint64_t>(8 * n0 + 1, 1024));
    if (ja.bloom0 == nullptr || ja.bloom0Log2 != b0Log2) {
      ja.bloom0 = (uint32_t*)devAlloc(ex, (1ULL << b0Log2) / 8);
      if (!ja.bloom0) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      ja.bloom0Log2 = b0Log2;
    }
    HIP_OK(ex, hipMemsetAsync(ja.bloom0, 0, (1ULL << ja.bloom0Log2) / 8,
                              ex->stream));
    if (getenv("GX_NO_BLOOM")) ja.bloom0Log2 = 0;
  }
  if (ja.keySet == nullptr || ja.keySetLog2 != wantLog2) {
    ja.keySet = (uint64_t*)devAlloc(ex, (1ULL << wantLog2) * 8);
    if (!ja.keySet) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    ja.keySetLog2 = wantLog2;
  }
  HIP_OK(ex, hipMemsetAsync(ja.keySet, 0xFF, (1ULL << ja.keySetLog2) * 8,
                            ex->stream));
  if ((rc = pushDesc())) return rc;
  if ((rc = phase(1))) return rc;

  // build1: count qualifying, size slots, init, fill
  if ((rc = phase(2))) return rc;
  uint64_t n1 = 0;
  if ((rc = readCounter(1, &n1))) return rc;
  wantLog2 = ceilLog2(std::max<uint64_t>(2 * n1 + 1, 64));
  if (!ja.chained && (ja.slots == nullptr || ja.slotsLog2 != wantLog2)) {
    ja.slots = (gxp::JoinAggSlot*)devAlloc(
        ex, (1ULL << wantLog2) * sizeof(gxp::JoinAggSlot));
    if (!ja.slots) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    ja.slotsLog2 = wantLog2;
  }
  ja.nSlots = ja.chained ? ja.build1.nRows : (1LL << ja.slotsLog2);
  int bloomLog2 = ceilLog2(std::max<uint64_t>(8 * n1 + 1, 1024));
  if (ja.bloom == nullptr || ja.bloomLog2 != bloomLog2) {
    ja.bloom = (uint32_t*)devAlloc(ex, (1ULL << bloomLog2) / 8);
    if (!ja.bloom) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    ja.bloomLog2 = bloomLog2;
  }
  HIP_OK(ex, hipMemsetAsync(ja.bloom, 0, (1ULL << ja.bloomLog2) / 8, ex->stream));
  if (getenv("GX_NO_BLOOM")) ja.bloomLog2 = 0;
  if ((rc = pushDesc())) return rc;
  if ((rc = phase(5))) return rc;  // init slots
  if ((rc = phase(3))) return rc;  // build
  if (!ja.chained) {
    // duplicate build keys? the unique-key insert flags kErrBadKey — retry
    // with the CHAINED slot layout (one slot per build1 row, heads+next
    // chains; each duplicate (key, payloads) row is its own group)
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    uint32_t ef = 0;
    HIP_OK(ex, hipMemcpy(&ef, ex->devErr, 4, hipMemcpyDeviceToHost));
    if (ef & 2u /*kErrBadKey*/) {
      ja.chained = 1;
      ja.b1HeadsLog2 = ceilLog2(std::max<uint64_t>(2 * n1 + 1, 64));
      ja.b1Heads = (uint32_t*)devAlloc(ex, (1ULL << ja.b1HeadsLog2) * 4);
      ja.b1Next = (uint32_t*)devAlloc(
          ex, std::max<int64_t>(ja.build1.nRows, 1) * 4);
      ja.slots = (gxp::JoinAggSlot*)devAlloc(
          ex, std::max<int64_t>(ja.build1.nRows, 1) *
                  sizeof(gxp::JoinAggSlot));
      if (!ja.b1Heads || !ja.b1Next || !ja.slots) {
        ex->err = "hipMalloc failed (chained join-agg)";
        return GX_ERR_INTERNAL;
      }
      ja.nSlots = ja.build1.nRows;
      // the chained variants run interpreted (no specialization yet)
      ex->jaJitProg = nullptr;
      ex->jaJitTried = true;
      ex->jaBuildProg = nullptr;
      ex->jaBuildTried = true;
      HIP_OK(ex, hipMemsetAsync(ja.b1Heads, 0, (1ULL << ja.b1HeadsLog2) * 4,
                                ex->stream));
      HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
      if (getenv("GX_DEBUG"))
        fprintf(stderr, "[gx] duplicate build keys -> chained join-agg\n");
      if ((rc = pushDesc())) return rc;
      if ((rc = phase(5))) return rc;  // re-init row-indexed slots
      if ((rc = phase(3))) return rc;  // chained build
    }
  }

  // specialize the probe kernel once per executor (gx_jit.cpp)
  if (!ex->jaJitTried && !getenv("GX_NO_JIT")) {
    ex->jaJitTried = true;
    std::string why;
    ex->jaJitProg = gxjit::compileJa(ja, &why);
    if (getenv("GX_DEBUG"))
      fprintf(stderr, "[gx] ja jit %s%s\n", ex->jaJitProg ? "ok" : "DISABLED: ",
              ex->jaJitProg ? "" : why.c_str());
  }

  // probe (timed — the dominant scan)
  hipEvent_t ev0, ev1;
  HIP_OK(ex, hipEventCreate(&ev0));
  HIP_OK(ex, hipEventCreate(&ev1));
  HIP_OK(ex, hipEventRecord(ev0, ex->stream));
  if ((rc = phase(4))) return rc;
  HIP_OK(ex, hipEventRecord(ev1, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  {
    float ms = 0;
    hipEventElapsedTime(&ms, ev0, ev1);
    ex->lastKernelMs = ms;
    hipEventDestroy(ev0);
    hipEventDestroy(ev1);
  }
  uint32_t errFlag = 0;
  HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
  if (errFlag == 256u && !ja.wide) {
    // narrow overflow: rebuild the accumulators and rerun wide
    ja.wide = 1;
    HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
    HIP_OK(ex, hipMemsetAsync(ja.counters + 2, 0, 8, ex->stream));
    if ((rc = pushDesc())) return rc;
    if ((rc = phase(5))) return rc;
    if ((rc = phase(3))) return rc;
    if ((rc = phase(4))) return rc;
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
  }
  errFlag &= ~256u;
  if (errFlag != 0) {
    ex->err = "device join error flag 0x" + std::to_string(errFlag);
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipMemcpy(&ex->lastSelCount, ja.counters + 2, 8,
                       hipMemcpyDeviceToHost));

  if (ja.chained) {
    // duplicate build rows with identical (key, payloads) are ONE group in
    // the reference — merge them before the top-N select
    if (gxp::gxJoinAggMergeDups(ex->devJa, ja, ex->stream) != 0) {
      ex->err = "dup-merge kernel failed";
      return GX_ERR_INTERNAL;
    }
  }

  // top-N selection: max -> 4096-bucket histogram -> threshold -> compact
  uint64_t* devMax = (uint64_t*)devAlloc(ex, 8);
  uint32_t* devHist = (uint32_t*)devAlloc(ex, 4096 * 4);
  uint64_t* devCount = (uint64_t*)devAlloc(ex, 8);
  if (!devMax || !devHist || !devCount) {
    ex->err = "hipMalloc failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipMemsetAsync(devMax, 0, 8, ex->stream));
  HIP_OK(ex, hipMemsetAsync(devHist, 0, 4096 * 4, ex->stream));
  HIP_OK(ex, hipMemsetAsync(devCount, 0, 8, ex->stream));
  // pass A of the 128-bit-capable select: max acc HI word -> topnShift so
  // key64 = acc128 >> shift is an order-preserving u64 (exact candidates
  // still compact with the full 128-bit acc; the host sorts them exactly)
  {
    uint64_t* devMaxHi = (uint64_t*)devAlloc(ex, 8);
    if (!devMaxHi) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemsetAsync(devMaxHi, 0, 8, ex->stream));
    if (gxp::gxJoinAggMaxHi(ex->devJa, ja, devMaxHi, ex->stream) != 0) {
      ex->err = "maxhi kernel failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    uint64_t maxHi = 0;
    HIP_OK(ex, hipMemcpy(&maxHi, devMaxHi, 8, hipMemcpyDeviceToHost));
    HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
    if (errFlag != 0) {
      ex->err = "negative revenue in device top-N unsupported this round";
      return GX_ERR_INTERNAL;
    }
    int bits = 0;
    while (bits < 64 && (maxHi >> bits) != 0) bits++;
    ja.topnShift = bits;
    if (bits) { if ((rc = pushDesc())) return rc; }
  }
  if (gxp::gxJoinAggMax(ex->devJa, ja, devMax, ex->stream) != 0) {
    ex->err = "max kernel failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  uint64_t maxRev = 0;
  HIP_OK(ex, hipMemcpy(&maxRev, devMax, 8, hipMemcpyDeviceToHost));
  int shift = 0;
  {
    int bits = 0;
    while (bits < 64 && (maxRev >> bits) != 0) bits++;  // bit63 can be set
    shift = bits > 12 ? bits - 12 : 0;
  }
  if (gxp::gxJoinAggHist(ex->devJa, ja, devHist, shift, ex->stream) != 0) {
    ex->err = "hist kernel failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  std::vector<uint32_t> hist(4096);
  HIP_OK(ex, hipMemcpy(hist.data(), devHist, 4096 * 4, hipMemcpyDeviceToHost));
  uint64_t need = (uint64_t)(ex->jaLimit + ex->jaOffset);
  uint64_t cum = 0;
  int thresholdBucket = 0;
  for (int b = 4095; b >= 0; b--) {
    cum += hist[b];
    if (cum >= need) {
      thresholdBucket = b;
      break;
    }
  }
  uint64_t cap = cum;
  std::vector<gxp::TopNOut> cand;
  if (cap > 0) {
    gxp::TopNOut* devOut =
        (gxp::TopNOut*)devAlloc(ex, cap * sizeof(gxp::TopNOut));
    if (!devOut) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    if (gxp::gxJoinAggCompact(ex->devJa, ja, devOut, devCount,
                              (uint64_t)thresholdBucket, shift, cap,
                              ex->stream) != 0) {
      ex->err = "compact kernel failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    uint64_t got = 0;
    HIP_OK(ex, hipMemcpy(&got, devCount, 8, hipMemcpyDeviceToHost));
    if (got > cap) got = cap;
    cand.resize(got);
    HIP_OK(ex, hipMemcpy(cand.data(), devOut, got * sizeof(gxp::TopNOut),
                         hipMemcpyDeviceToHost));
  }

  // host: sort candidates by the TopN keys, slice, emit
  size_t nGroup = ex->jaGroupSrc.size();
  auto groupVal = [&](const gxp::TopNOut& c, size_t g) -> uint64_t {
    switch (ex->jaGroupSrc[g]) {
      case 0: return c.key;
      case 1: return c.payload0;
      default: return (uint64_t)c.payload1;
    }
  };
  auto cmpKeys = [&](const gxp::TopNOut& a, const gxp::TopNOut& b) -> bool {
    for (auto& [col, desc] : ex->jaSortKeys) {
      int cres = 0;
      if (col == (int)nGroup) {  // the sum column: int128 compare
        __int128 x = ((__int128)a.accHi << 64) | a.accLo;
        __int128 y = ((__int128)b.accHi << 64) | b.accLo;
        cres = x < y ? -1 : (x > y ? 1 : 0);
      } else {
        int t = ex->jaGroupType[col];
        uint64_t x = groupVal(a, col), y = groupVal(b, col);
        if (t == GX_TYPE_TIME) {
          x &= ~0xFULL;
          y &= ~0xFULL;
          cres = x < y ? -1 : (x > y ? 1 : 0);
        } else {
          int64_t sx = (int64_t)x, sy = (int64_t)y;
          cres = sx < sy ? -1 : (sx > sy ? 1 : 0);
        }
      }
      if (desc) cres = -cres;
      if (cres != 0) return cres < 0;
    }
    return false;
  };
  size_t want = std::min<size_t>(cand.size(), (size_t)(ex->jaLimit + ex->jaOffset));
  std::partial_sort(cand.begin(), cand.begin() + want, cand.end(), cmpKeys);
  ex->resultRows.clear();
  for (size_t i = (size_t)ex->jaOffset; i < want; i++) {
    const gxp::TopNOut& c = cand[i];
    std::vector<OutRowVal> row;
    for (size_t g = 0; g < nGroup; g++) {
      OutRowVal v;
      v.type = ex->jaGroupType[g];
      v.u64 = groupVal(c, g);
      v.i64 = (int64_t)v.u64;
      row.push_back(std::move(v));
    }
    OutRowVal v;
    v.type = GX_TYPE_DECIMAL;
    __int128 acc = ((__int128)c.accHi << 64) | c.accLo;
    v.dec = decFromUnits(acc, ex->jaValueScale);
    v.dec.Round(&v.dec, ex->jaAggFrac, gxp::ModeHalfUp);
    row.push_back(std::move(v));
    ex->resultRows.push_back(std::move(row));
  }
  return GX_OK;
}

// ---------------- standalone hash join execution ----------------

// gather nCols columns of srcTab through a match/survivor index into
// out->cols[dstBase..): fixed-width, dense char (identity offsets), general
// varlen (two-pass), and null bitmaps
// gather one column's null bitmap through the match index (allocates the
// output bitmap; forceNulls covers null-extended outer-join rows over a
// source with no bitmap)
static int32_t gatherColNulls(gx_exec* ex, const gxp::DevCol& src,
                              const uint32_t* idx, uint64_t total,
                              gxp::DevCol* dst, bool forceNulls) {
  if ((src.hasNulls && src.nullBitmap) || forceNulls) {
    dst->nullBitmap = (uint8_t*)devAlloc(ex, (total + 7) / 8);
    if (!dst->nullBitmap) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    if (gxp::gxGatherNulls(src.hasNulls ? src.nullBitmap : nullptr, idx,
                           dst->nullBitmap, (int64_t)total, ex->stream) != 0) {
      ex->err = "null gather launch failed";
      return GX_ERR_INTERNAL;
    }
    dst->hasNulls = 1;
  } else {
    dst->nullBitmap = nullptr;
    dst->hasNulls = 0;
  }
  return GX_OK;
}

// general varlen gather through an index: lengths -> exclusive scan -> byte
// copy. Fills dst's data, offsets and denseOffsets; the null bitmap is the
// caller's.
static int32_t gatherVarlenCol(gx_exec* ex, const gxp::DevCol& src,
                               const uint32_t* idx, uint64_t total,
                               gxp::DevCol& dst) {
  int64_t* lens = (int64_t*)devAlloc(ex, total * 8);
  dst.offsets = (int64_t*)devAlloc(ex, (total + 1) * 8);
  if (!lens || !dst.offsets) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  if (gxp::gxGatherVarlenLens(src.offsets, idx, lens, (int64_t)total,
                              ex->stream) != 0) {
    ex->err = "varlen lens launch failed";
    return GX_ERR_INTERNAL;
  }
  size_t tmpBytes = 0;
  gxp::gxExclusiveSumI64(lens, dst.offsets, (int64_t)total, nullptr,
                         &tmpBytes, ex->stream);
  void* tmp = devAlloc(ex, std::max<size_t>(tmpBytes, 1));
  if (!tmp) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  HIP_OK(ex, hipMemsetAsync(dst.offsets, 0, 8, ex->stream));
  if (gxp::gxExclusiveSumI64(lens, dst.offsets, (int64_t)total, tmp,
                             &tmpBytes, ex->stream) != 0) {
    ex->err = "varlen offsets scan failed";
    return GX_ERR_INTERNAL;
  }
  int64_t totalBytes = 0;
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  HIP_OK(ex, hipMemcpy(&totalBytes, dst.offsets + total, 8,
                       hipMemcpyDeviceToHost));
  dst.data = devAlloc(ex, std::max<int64_t>(totalBytes, 1));
  if (!dst.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  if (gxp::gxGatherVarlenBytes((const uint8_t*)src.data, src.offsets,
                               idx, dst.offsets, (uint8_t*)dst.data,
                               (int64_t)total, ex->stream) != 0) {
    ex->err = "varlen bytes launch failed";
    return GX_ERR_INTERNAL;
  }
  dst.denseOffsets = 0;
  return GX_OK;
}

static int32_t gatherCols(gx_exec* ex, const gxp::DevTable& srcTab,
                          const uint32_t* idx, uint64_t total,
                          gxp::DevTable* out, int dstBase,
                          bool forceNulls = false) {
  for (int c = 0; c < srcTab.nCols; c++) {
    const gxp::DevCol& src = srcTab.cols[c];
    gxp::DevCol& dst = out->cols[dstBase + c];
    if (src.type == GX_TYPE_STRING && !src.denseOffsets) {
      int32_t vrc = gatherVarlenCol(ex, src, idx, total, dst);
      if (vrc) return vrc;
    } else {
      int es = src.type == GX_TYPE_DECIMAL ? 40
               : (src.type == GX_TYPE_STRING ? 1 : 8);
      dst.data = devAlloc(ex, (size_t)total * es + 16);
      if (!dst.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      if (gxp::gxSortGatherCol(src.data, dst.data, idx, (int64_t)total, es,
                               ex->stream) != 0) {
        ex->err = "gather launch failed";
        return GX_ERR_INTERNAL;
      }
      if (src.type == GX_TYPE_STRING) {
        dst.offsets = (int64_t*)devAlloc(ex, (total + 1) * 8);
        if (!dst.offsets) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        if (gxp::gxIotaOffsets(dst.offsets, (int64_t)total + 1, ex->stream) != 0) {
          ex->err = "offsets launch failed";
          return GX_ERR_INTERNAL;
        }
        dst.denseOffsets = 1;
      }
    }
    int32_t rc = gatherColNulls(ex, src, idx, total, &dst, forceNulls);
    if (rc) return rc;
  }
  return GX_OK;
}

// row-pack variant: >= 2 fixed-width columns pack row-major once (sequential
// pass over the source), then the random per-output-row fetch touches one
// packed row — one or two cache lines — instead of one line PER COLUMN.
// General varlen columns and null bitmaps keep the per-column paths.
static int32_t gatherColsAuto(gx_exec* ex, const gxp::DevTable& srcTab,
                              const uint32_t* idx, uint64_t total,
                              gxp::DevTable* out, int dstBase,
                              bool forceNulls) {
  gxp::RowPackDesc pd{};
  int stride = 0;
  std::vector<int> cols;
  for (int pass = 0; pass < 2; pass++) {  // 8-aligned widths first, chars last
    for (int c = 0; c < srcTab.nCols; c++) {
      const gxp::DevCol& src = srcTab.cols[c];
      int w = src.type == GX_TYPE_DECIMAL  ? 40
              : src.type == GX_TYPE_STRING ? (src.denseOffsets ? 1 : 0)
                                           : 8;
      if (w == 0 || (pass == 0) != (w >= 8)) continue;
      pd.src[pd.nCols] = src.data;
      pd.width[pd.nCols] = w;
      pd.off[pd.nCols] = stride;
      cols.push_back(c);
      stride += w;
      pd.nCols++;
    }
  }
  // worth packing only when the sequential pack pass is cheaper than the
  // per-column random line fetches it saves
  if (pd.nCols < 2 || srcTab.nRows > 2 * (int64_t)total)
    return gatherCols(ex, srcTab, idx, total, out, dstBase, forceNulls);
  pd.stride = (stride + 7) & ~7;
  pd.nRows = srcTab.nRows;
  pd.idx = idx;
  pd.total = (int64_t)total;
  pd.staging = (uint8_t*)devAlloc(ex, (size_t)pd.nRows * pd.stride + 16);
  if (!pd.staging) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  for (int k = 0; k < pd.nCols; k++) {
    int c = cols[k];
    const gxp::DevCol& src = srcTab.cols[c];
    gxp::DevCol& dst = out->cols[dstBase + c];
    dst.data = devAlloc(ex, (size_t)total * pd.width[k] + 16);
    if (!dst.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    pd.dst[k] = dst.data;
    if (src.type == GX_TYPE_STRING) {  // dense char(1)
      dst.offsets = (int64_t*)devAlloc(ex, (total + 1) * 8);
      if (!dst.offsets) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      if (gxp::gxIotaOffsets(dst.offsets, (int64_t)total + 1, ex->stream) != 0) {
        ex->err = "offsets launch failed";
        return GX_ERR_INTERNAL;
      }
      dst.denseOffsets = 1;
    }
    int32_t rc = gatherColNulls(ex, src, idx, total, &dst, forceNulls);
    if (rc) return rc;
  }
  if (gxp::gxPackRows(pd, ex->stream) != 0 ||
      gxp::gxUnpackRows(pd, ex->stream) != 0) {
    ex->err = "row-pack gather launch failed";
    return GX_ERR_INTERNAL;
  }
  // remaining (general varlen) columns via the per-column path
  for (int c = 0; c < srcTab.nCols; c++) {
    const gxp::DevCol& src = srcTab.cols[c];
    if (!(src.type == GX_TYPE_STRING && !src.denseOffsets)) continue;
    gxp::DevTable one{};
    one.nCols = 1;
    one.cols[0] = src;
    one.nRows = srcTab.nRows;
    gxp::DevTable oneOut{};
    oneOut.cols[0] = out->cols[dstBase + c];
    int32_t rc = gatherCols(ex, one, idx, total, &oneOut, 0, forceNulls);
    if (rc) return rc;
    out->cols[dstBase + c] = oneOut.cols[0];
  }
  return GX_OK;
}

// run one join stage: chain build -> count -> fill -> [post filter] ->
// gather into st.out. Sides come from bound sources (materialized once) or
// previous stages' outputs.
static int32_t runJoinStage(gx_exec* ex, gx_exec::JoinStage& st, bool isRoot) {
  // a per-run copy: the run's buffers and the effective join type a
  // null-aware join settles on must not outlive it in st.hj
  gxp::HashJoinDesc hj = st.hj;
  hj.build = st.srcB >= 0 ? st.buildTab : ex->joinStages[st.buildStage].out;
  hj.probe = st.srcP >= 0 ? st.probeTab : ex->joinStages[st.probeStage].out;
  int64_t nb = hj.build.nRows;
  if (nb >= 0xFFFFFFFFLL || hj.probe.nRows > 0xFFFFFFFFLL) {
    ex->err = "join sides > 2^32 rows unsupported this round";
    return GX_ERR_INVALID;
  }
  hipEvent_t ev0, ev1, evB, evC, evF;
  HIP_OK(ex, hipEventCreate(&ev0));
  HIP_OK(ex, hipEventCreate(&ev1));
  HIP_OK(ex, hipEventCreate(&evB));
  HIP_OK(ex, hipEventCreate(&evC));
  HIP_OK(ex, hipEventCreate(&evF));
  HIP_OK(ex, hipEventRecord(ev0, ex->stream));
  // chained table: heads (2x rows, pow2) + per-row next links
  hj.headsLog2 = ceilLog2(std::max<uint64_t>(2 * (uint64_t)nb + 1, 64));
  hj.heads = (uint32_t*)devAlloc(ex, (1ULL << hj.headsLog2) * 4);
  hj.next = (uint32_t*)devAlloc(ex, std::max<int64_t>(nb, 1) * 4);
  if (!hj.heads || !hj.next) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  if (hj.joinType == 2) {  // right outer: per-build-row matched flags
    size_t words = ((size_t)nb + 31) / 32;
    hj.matched = (uint32_t*)devAlloc(ex, std::max<size_t>(words * 4, 4));
    if (!hj.matched) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemsetAsync(hj.matched, 0, std::max<size_t>(words * 4, 4),
                              ex->stream));
  }
  // deterministic-fill scratch: per-row walk cache + per-64-row-tile emit
  // counts scanned into bases (no shared-cursor atomics in the fill pass)
  const int64_t nProbe = hj.probe.nRows;
  const int64_t nTiles = (nProbe + 63) / 64;
  hj.hits = (uint32_t*)devAlloc(ex, std::max<int64_t>(nProbe, 1) * 4);
  hj.tileCounts = (int64_t*)devAlloc(ex, std::max<int64_t>(nTiles, 1) * 8);
  hj.tileBases = (int64_t*)devAlloc(ex, (std::max<int64_t>(nTiles, 1) + 1) * 8);
  if (!hj.hits || !hj.tileCounts || !hj.tileBases) {
    ex->err = "hipMalloc failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipMemsetAsync(hj.heads, 0, (1ULL << hj.headsLog2) * 4, ex->stream));
  HIP_OK(ex, hipMemsetAsync(hj.counters, 0, 24, ex->stream));
  HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
  HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj), hipMemcpyHostToDevice,
                            ex->stream));
  if (gxp::gxHashJoinPhase(0, ex->devHj, hj, ex->stream) != 0) {
    ex->err = "join kernel launch failed";
    return GX_ERR_INTERNAL;
  }
  if (hj.joinType == 5 || hj.joinType == 7) {
    // null-aware anti semi (x NOT IN ...): two build scalars decide the
    // shape (null_aware NAASJ, hash_join_v1.go:599):
    //   no passing build rows  -> NOT IN (empty) is TRUE for EVERY probe
    //                             row incl. NULL keys == plain anti semi
    //   any NULL build key     -> NOT IN is never TRUE -> empty output
    //   else                   -> anti semi that also rejects NULL probe
    //                             keys (the kernels' joinType==5 paths)
    uint64_t* bstats = (uint64_t*)devAlloc(ex, 16);
    if (!bstats) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemsetAsync(bstats, 0, 16, ex->stream));
    if (gxp::gxHjBuildStats(ex->devHj, hj, bstats, ex->stream) != 0) {
      ex->err = "join build-stats launch failed";
      return GX_ERR_INTERNAL;
    }
    uint64_t hstats[2] = {0, 0};
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    HIP_OK(ex, hipMemcpy(hstats, bstats, 16, hipMemcpyDeviceToHost));
    if (ex->joinSpill) {  // hj.build is one partition: take the whole side's
      hstats[0] = ex->spillBuildPass;
      hstats[1] = ex->spillBuildNullKeys;
    }
    if (hj.joinType == 5) {
      if (hstats[0] == 0) {
        hj.joinType = 4;  // empty valid set: every probe row qualifies
      } else if (hstats[1] > 0) {
        hj.probe.nRows = 0;  // a NULL y: no probe row can qualify
      }
    } else {  // null-aware left outer semi: no-match flag NULL conditions
      hj.naNullIfKeyNull = hstats[0] > 0 ? 1 : 0;
      hj.naNullAlways = hstats[1] > 0 ? 1 : 0;
    }
    HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj),
                              hipMemcpyHostToDevice, ex->stream));
  }
  HIP_OK(ex, hipEventRecord(evB, ex->stream));
  if (gxp::gxHashJoinPhase(1, ex->devHj, hj, ex->stream) != 0) {
    ex->err = "join kernel launch failed";
    return GX_ERR_INTERNAL;
  }
  if (hj.joinType == 2 &&
      gxp::gxHashJoinPhase(4, ex->devHj, hj, ex->stream) != 0) {
    ex->err = "join unmatched-count launch failed";
    return GX_ERR_INTERNAL;
  }
  // scan tile counts -> fill bases (tileBases[nTiles] = matched total, which
  // also seeds the unmatched-drain cursor for right outer)
  if (nTiles > 0) {
    size_t tmpBytes = 0;
    gxp::gxExclusiveSumI64(hj.tileCounts, hj.tileBases, nTiles, nullptr,
                           &tmpBytes, ex->stream);
    void* tmp = devAlloc(ex, std::max<size_t>(tmpBytes, 1));
    if (!tmp) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemsetAsync(hj.tileBases, 0, 8, ex->stream));
    if (gxp::gxExclusiveSumI64(hj.tileCounts, hj.tileBases, nTiles, tmp,
                               &tmpBytes, ex->stream) != 0) {
      ex->err = "tile-base scan failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipMemcpyAsync(&hj.counters[1], &hj.tileBases[nTiles], 8,
                              hipMemcpyDeviceToDevice, ex->stream));
  }
  HIP_OK(ex, hipEventRecord(evC, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  uint64_t total = 0;
  HIP_OK(ex, hipMemcpy(&total, hj.counters, 8, hipMemcpyDeviceToHost));
  uint32_t errFlag = 0;
  HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
  if (errFlag != 0) {
    ex->err = "device join error flag 0x" + std::to_string(errFlag);
    return GX_ERR_INTERNAL;
  }
  if (total > 0x7FFFFFFFULL) {
    ex->err = "join output > 2^31 rows unsupported this round";
    return GX_ERR_INVALID;
  }
  // output table (schema fixed at compile; buffers per run)
  setTableMeta(&st.out, st.types, st.fracs);
  st.out.nRows = 0;
  if (total > 0) {
    hj.outBuild = (uint32_t*)devAlloc(ex, total * 4);
    hj.outProbe = (uint32_t*)devAlloc(ex, total * 4);
    if (!hj.outBuild || !hj.outProbe) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj),
                              hipMemcpyHostToDevice, ex->stream));
    if (gxp::gxHashJoinPhase(2, ex->devHj, hj, ex->stream) != 0) {
      ex->err = "join fill launch failed";
      return GX_ERR_INTERNAL;
    }
    if (hj.joinType == 2 &&
        gxp::gxHashJoinPhase(5, ex->devHj, hj, ex->stream) != 0) {
      ex->err = "join unmatched-fill launch failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipEventRecord(evF, ex->stream));
    // post-join filter (other conditions): compact surviving pairs before
    // the gather so rejected rows never touch the output
    const uint32_t* gatherB = hj.outBuild;
    const uint32_t* gatherP = hj.outProbe;
    if (hj.nPost > 0) {
      hj.nPairs = (int64_t)total;
      hj.outBuild2 = (uint32_t*)devAlloc(ex, total * 4);
      hj.outProbe2 = (uint32_t*)devAlloc(ex, total * 4);
      if (!hj.outBuild2 || !hj.outProbe2) {
        ex->err = "hipMalloc failed";
        return GX_ERR_INTERNAL;
      }
      HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj),
                                hipMemcpyHostToDevice, ex->stream));
      if (gxp::gxHashJoinPhase(3, ex->devHj, hj, ex->stream) != 0) {
        ex->err = "join filter launch failed";
        return GX_ERR_INTERNAL;
      }
      HIP_OK(ex, hipStreamSynchronize(ex->stream));
      uint64_t total2 = 0;
      HIP_OK(ex, hipMemcpy(&total2, hj.counters + 2, 8, hipMemcpyDeviceToHost));
      total = total2;
      gatherB = hj.outBuild2;
      gatherP = hj.outProbe2;
    }
    // gather every output column through its side's match index
    if (total > 0) {
      gxp::DevTable bsub = hj.build;
      gxp::DevTable psub = hj.probe;
      int32_t rc;
      if (hj.joinType >= 3) {
        // semi family: probe (outer) columns only; 6/7 add the scalar col
        rc = gatherCols(ex, psub, gatherP, total, &st.out, 0, false);
        if (rc == GX_OK && hj.joinType >= 6) {
          gxp::DevCol& fc = st.out.cols[psub.nCols];
          fc.data = devAlloc(ex, (size_t)total * 8 + 16);
          fc.nullBitmap = (uint8_t*)devAlloc(ex, (total + 7) / 8 + 1);
          if (!fc.data || !fc.nullBitmap) {
            ex->err = "hipMalloc failed";
            return GX_ERR_INTERNAL;
          }
          fc.hasNulls = 1;  // flag 2 rows (undecidable x IN S) are NULL
          if (gxp::gxHjFlagCol(gatherB, (int64_t)total, (int64_t*)fc.data,
                               fc.nullBitmap, ex->stream) != 0) {
            ex->err = "flag column launch failed";
            return GX_ERR_INTERNAL;
          }
        }
      } else {
        // outer joins carry null-extended rows on the inner side; the build
        // side (the random-access gather) goes through the row-pack path
        rc = gatherColsAuto(ex, bsub, gatherB, total, &st.out, 0,
                            hj.joinType == 1);
        if (rc == GX_OK)
          rc = gatherCols(ex, psub, gatherP, total, &st.out, hj.build.nCols,
                          hj.joinType == 2);
      }
      if (rc) return rc;
    }
  }
  HIP_OK(ex, hipEventRecord(ev1, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  {
    float ms = 0;
    hipEventElapsedTime(&ms, ev0, ev1);
    ex->lastKernelMs += ms;
    if (isRoot) ex->lastSelCount = total;
    if (getenv("GX_DEBUG")) {
      float mb = 0, mc = 0, mf = 0;
      hipEventElapsedTime(&mb, ev0, evB);
      hipEventElapsedTime(&mc, evB, evC);
      if (total > 0) hipEventElapsedTime(&mf, evC, evF);
      fprintf(stderr,
              "[gx] hj%s build=%.3fms count=%.3fms fill=%.3fms gather=%.3fms "
              "total=%.3fms matches=%llu\n",
              isRoot ? "" : " (inner)", mb, mc, mf, ms - mb - mc - mf, ms,
              (unsigned long long)total);
    }
    hipEventDestroy(ev0);
    hipEventDestroy(ev1);
    hipEventDestroy(evB);
    hipEventDestroy(evC);
    hipEventDestroy(evF);
  }
  st.out.nRows = (int64_t)total;
  return GX_OK;
}


// ---------------- out-of-core join (hash_join_spill.go analog) ----------------

static int64_t hbmBudgetBytes() {
  if (const char* e = getenv("GX_HBM_BUDGET")) return atoll(e);
  size_t freeB = 0, totalB = 0;
  if (hipMemGetInfo(&freeB, &totalB) == hipSuccess)
    return (int64_t)(freeB / 100 * 92);
  return INT64_MAX;
}

// rough resident bytes per row of a source schema (varlen estimated at the
// generator's ~1 B payload + the 8 B offsets entry; bound chunks of long
// strings under-estimate, which only delays the spill until allocation
// actually fails — never wrong results)
static int64_t schemaRowBytes(const PNode& srcN) {
  int64_t b = 0;
  for (int t : srcN.colTypes)
    b += t == GX_TYPE_DECIMAL ? 40 : (t == GX_TYPE_STRING ? 9 : 8);
  return b;
}

static int64_t bindingRows(gx_exec* ex, int srcId) {
  auto it = ex->bindings.find(srcId);
  if (it == ex->bindings.end()) return 0;
  if (it->second.haveChunks) {
    int64_t n = 0;
    for (auto& ch : it->second.chunks) n += ch.empty() ? 0 : ch[0].length;
    return n;
  }
  return it->second.tpchRows;
}

// hash-partition one side into host-RAM runs, streaming the source in
// budget-bounded row slices (generator sources re-generate per slice; bound
// chunks upload once — their size is the caller's to bound)
static int32_t partitionJoinSide(gx_exec* ex, gx_exec::JoinStage& st,
                                 int side, int nParts, int64_t sliceRows,
                                 std::vector<JoinPart>* parts) {
  int srcId = side == 0 ? st.srcB : st.srcP;
  const PNode& srcN = ex->plan.nodes[srcId];
  Binding& b = ex->bindings[srcId];
  int nc = (int)srcN.colTypes.size();
  parts->assign(nParts, JoinPart{});
  if (side == 0) ex->spillBuildPass = ex->spillBuildNullKeys = 0;
  for (auto& jp : *parts) {
    jp.colData.resize(nc);
    jp.colOffsets.resize(nc);
    jp.nullBytes.resize(nc);
    for (int c = 0; c < nc; c++)
      if (srcN.colTypes[c] == GX_TYPE_STRING) jp.colOffsets[c].push_back(0);
  }
  const int64_t saveRows = b.tpchRows, saveOff = b.tpchRowOffset,
                saveTot = b.tpchTotalRows;
  int64_t done = 0;
  bool chunksDone = false;  // a chunk-bound side uploads once, rows or none
  int32_t rc = GX_OK;
  for (;;) {
    size_t mark = ex->devBufs.size();
    gxp::DevTable tab{};
    if (b.haveChunks) {
      if (chunksDone) break;
      chunksDone = true;
      rc = materializeTable(ex, srcId, &tab);
      if (rc) break;
      done = tab.nRows;
    } else {
      if (done >= saveRows) break;
      int64_t n = std::min(sliceRows, saveRows - done);
      b.tpchRowOffset = saveOff + done;
      b.tpchRows = n;
      b.tpchTotalRows = saveTot > 0 ? saveTot : saveRows;
      rc = materializeTable(ex, srcId, &tab);
      if (rc) break;
      done += n;
    }
    int64_t n = tab.nRows;
    if (n == 0) { freeSince(ex, mark); continue; }
    uint32_t* devPid = (uint32_t*)devAlloc(ex, (size_t)n * 4);
    if (!devPid) { ex->err = "hipMalloc failed"; rc = GX_ERR_INTERNAL; break; }
    gxp::HashJoinDesc hj2 = st.hj;
    if (side == 0) hj2.build = tab;
    else hj2.probe = tab;
    hipError_t he = hipMemcpyAsync(ex->devHj, &hj2, sizeof(hj2),
                                   hipMemcpyHostToDevice, ex->stream);
    if (he != hipSuccess ||
        gxp::gxHjPartIds(ex->devHj, hj2, side, nParts, devPid,
                         ex->stream) != 0) {
      ex->err = "partition-id launch failed";
      rc = GX_ERR_INTERNAL;
      break;
    }
    if (hipStreamSynchronize(ex->stream) != hipSuccess) {
      ex->err = "partition sync failed";
      rc = GX_ERR_INTERNAL;
      break;
    }
    std::vector<uint32_t> pid(n);
    hipMemcpy(pid.data(), devPid, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (side == 0 && (st.hj.joinType == 5 || st.hj.joinType == 7)) {
      // the null-aware joins' two build scalars cover the whole build side,
      // not one partition: count them per slice while it is on the device
      uint64_t* bstats = (uint64_t*)devAlloc(ex, 16);
      uint64_t hstats[2] = {0, 0};
      if (!bstats || hipMemsetAsync(bstats, 0, 16, ex->stream) != hipSuccess ||
          gxp::gxHjBuildStats(ex->devHj, hj2, bstats, ex->stream) != 0 ||
          hipStreamSynchronize(ex->stream) != hipSuccess ||
          hipMemcpy(hstats, bstats, 16, hipMemcpyDeviceToHost) != hipSuccess) {
        ex->err = "join build-stats launch failed";
        rc = GX_ERR_INTERNAL;
        break;
      }
      ex->spillBuildPass += hstats[0];
      ex->spillBuildNullKeys += hstats[1];
    }
    // download the slice
    std::vector<std::vector<uint8_t>> hData(nc);
    std::vector<std::vector<int64_t>> hOff(nc);
    std::vector<std::vector<uint8_t>> hNull(nc);
    for (int c = 0; c < nc; c++) {
      const gxp::DevCol& col = tab.cols[c];
      if (col.type == GX_TYPE_STRING) {
        hOff[c].resize(n + 1);
        hipMemcpy(hOff[c].data(), col.offsets, (size_t)(n + 1) * 8,
                  hipMemcpyDeviceToHost);
        hData[c].resize(std::max<int64_t>(hOff[c][n], 1));
        if (hOff[c][n] > 0)
          hipMemcpy(hData[c].data(), col.data, (size_t)hOff[c][n],
                    hipMemcpyDeviceToHost);
      } else {
        hData[c].resize((size_t)n * col.elemSize);
        hipMemcpy(hData[c].data(), col.data, hData[c].size(),
                  hipMemcpyDeviceToHost);
      }
      if (col.hasNulls && col.nullBitmap) {
        hNull[c].resize((n + 7) / 8);
        hipMemcpy(hNull[c].data(), col.nullBitmap, hNull[c].size(),
                  hipMemcpyDeviceToHost);
      }
    }
    freeSince(ex, mark);
    // split rows into partitions on the host
    for (int64_t r = 0; r < n; r++) {
      JoinPart& jp = (*parts)[pid[r]];
      for (int c = 0; c < nc; c++) {
        if (srcN.colTypes[c] == GX_TYPE_STRING) {
          int64_t s = hOff[c][r], e2 = hOff[c][r + 1];
          jp.colData[c].insert(jp.colData[c].end(), hData[c].begin() + s,
                               hData[c].begin() + e2);
          jp.colOffsets[c].push_back((int64_t)jp.colData[c].size());
        } else {
          int es = srcN.colTypes[c] == GX_TYPE_DECIMAL ? 40 : 8;
          jp.colData[c].insert(jp.colData[c].end(),
                               hData[c].begin() + (size_t)r * es,
                               hData[c].begin() + (size_t)(r + 1) * es);
        }
        if (!hNull[c].empty()) {
          if (jp.nullBytes[c].empty() && jp.n > 0)
            jp.nullBytes[c].assign((size_t)jp.n, 1);
          if (!hNull[c].empty())
            jp.nullBytes[c].push_back((hNull[c][r / 8] >> (r % 8)) & 1);
        } else if (!jp.nullBytes[c].empty()) {
          jp.nullBytes[c].push_back(1);
        }
      }
      jp.n++;
    }
  }
  b.tpchRows = saveRows;
  b.tpchRowOffset = saveOff;
  b.tpchTotalRows = saveTot;
  return rc;
}

// upload one host partition as a resident device table
static int32_t uploadJoinPart(gx_exec* ex, const PNode& srcN,
                              const JoinPart& jp, gxp::DevTable* tab) {
  int nc = (int)srcN.colTypes.size();
  tab->nCols = nc;
  tab->nRows = jp.n;
  int64_t n = jp.n;
  for (int c = 0; c < nc; c++) {
    gxp::DevCol& col = tab->cols[c];
    setDevColMeta(&col, srcN.colTypes[c], srcN.colFracs[c]);
    // tab persists across partitions: clear the previous partition's (freed)
    // buffers so a no-NULL partition cannot inherit a stale bitmap
    col.data = nullptr;
    col.offsets = nullptr;
    col.nullBitmap = nullptr;
    col.hasNulls = 0;
    col.denseOffsets = 0;
    if (srcN.colTypes[c] == GX_TYPE_STRING) {
      col.offsets = (int64_t*)devAlloc(ex, (size_t)(n + 1) * 8);
      col.data = devAlloc(ex, std::max<size_t>(jp.colData[c].size(), 1));
      if (!col.offsets || !col.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      hipMemcpy(col.offsets, jp.colOffsets[c].data(), (size_t)(n + 1) * 8,
                hipMemcpyHostToDevice);
      if (!jp.colData[c].empty())
        hipMemcpy(col.data, jp.colData[c].data(), jp.colData[c].size(),
                  hipMemcpyHostToDevice);
      // dense = every value exactly one byte (offsets are the identity
      // ramp), as uploadBoundChunks checks it; lengths {0, 2} also sum to n
      bool dense = true;
      for (int64_t i = 0; i <= n && dense; i++)
        dense = jp.colOffsets[c][i] == i;
      col.denseOffsets = dense ? 1 : 0;
    } else {
      col.data = devAlloc(ex, std::max<size_t>(jp.colData[c].size(), 1) + 16);
      if (!col.data) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      if (!jp.colData[c].empty())
        hipMemcpy(col.data, jp.colData[c].data(), jp.colData[c].size(),
                  hipMemcpyHostToDevice);
    }
    if (!jp.nullBytes[c].empty()) {
      std::vector<uint8_t> bm((n + 7) / 8, 0);
      bool anyNull = false;
      for (int64_t r = 0; r < n; r++) {
        if (jp.nullBytes[c][r]) bm[r / 8] |= 1 << (r % 8);
        else anyNull = true;
      }
      if (anyNull) {
        col.nullBitmap = (uint8_t*)devAlloc(ex, bm.size());
        if (!col.nullBitmap) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
        hipMemcpy(col.nullBitmap, bm.data(), bm.size(), hipMemcpyHostToDevice);
        col.hasNulls = 1;
      }
    }
  }
  return GX_OK;
}

// run the next non-empty partition's join; leaves its output in desc.table
// (nRows 0 once exhausted)
static int32_t joinSpillAdvance(gx_exec* ex) {
  gx_exec::JoinStage& st = ex->joinStages[0];
  while (++ex->joinSpillCur < (int)ex->spillB.size()) {
    freeSince(ex, ex->joinSpillMark);
    int p = ex->joinSpillCur;
    if (ex->spillB[p].n == 0 && ex->spillP[p].n == 0) continue;
    const PNode& bN = ex->plan.nodes[st.srcB];
    const PNode& pN = ex->plan.nodes[st.srcP];
    int32_t rc = uploadJoinPart(ex, bN, ex->spillB[p], &st.buildTab);
    if (rc == GX_OK) rc = uploadJoinPart(ex, pN, ex->spillP[p], &st.probeTab);
    if (rc) return rc;
    st.inputsReady = true;
    if (getenv("GX_DEBUG")) {
      int64_t bk = 0, pk = 0;
      if (ex->spillB[p].n > 0 && ex->spillB[p].colData[0].size() >= 8)
        std::memcpy(&bk, ex->spillB[p].colData[0].data(), 8);
      if (ex->spillP[p].n > 0 && ex->spillP[p].colData[0].size() >= 8)
        std::memcpy(&pk, ex->spillP[p].colData[0].data(), 8);
      fprintf(stderr,
              "[gx] spill part %d: build %lld (k0=%lld) probe %lld (k0=%lld)\n",
              p, (long long)ex->spillB[p].n, (long long)bk,
              (long long)ex->spillP[p].n, (long long)pk);
    }
    rc = runJoinStage(ex, st, true);
    if (rc) return rc;
    ex->joinSpillMatches += ex->lastSelCount;
    for (int c = 0; c < st.out.nCols; c++)
      ex->desc.table.cols[c] = st.out.cols[c];
    ex->desc.table.nCols = st.out.nCols;
    ex->desc.table.nRows = st.out.nRows;
    ex->srcPos = 0;
    if (st.out.nRows == 0) continue;
    return GX_OK;
  }
  ex->desc.table.nRows = 0;
  ex->srcPos = 0;
  ex->lastSelCount = ex->joinSpillMatches;
  return GX_OK;
}

static int32_t runHashJoin(gx_exec* ex) {
  if (!ex->deviceReady) {
    if (!gpuAvailable()) {
      ex->err = "no MI355X visible: the product engine has no CPU fallback "
                "(GX_ERR_NO_GPU)";
      return GX_ERR_NO_GPU;
    }
    if (ex->device >= 0) hipSetDevice(ex->device);
    HIP_OK(ex, hipStreamCreate(&ex->stream));
    ex->devErr = (uint32_t*)devAllocP(ex, 4);
    ex->devHj = (gxp::HashJoinDesc*)devAllocP(ex, sizeof(gxp::HashJoinDesc));
    if (!ex->devErr || !ex->devHj) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
    ex->deviceReady = true;
  }
  ex->lastKernelMs = 0;
  // out-of-core: when build + probe + output would exceed the HBM budget
  // (GX_HBM_BUDGET overrides the free-memory estimate), hash-partition both
  // sides to host RAM and join partition-wise (hash_join_spill.go analog).
  // Single-stage source-fed joins only; partitions persist across re-opens.
  if (ex->joinStages.size() == 1 && ex->kind != ExecKind::AGG_OVER_JOIN &&
      ex->joinStages[0].srcB >= 0 && ex->joinStages[0].srcP >= 0) {
    gx_exec::JoinStage& st0 = ex->joinStages[0];
    if (!st0.hj.counters) {
      st0.hj.counters = (uint64_t*)devAllocP(ex, 3 * 8);
      if (!st0.hj.counters) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    }
    st0.hj.errorFlag = ex->devErr;
    if (!ex->joinSpill && !st0.inputsReady) {
      int64_t rbB = schemaRowBytes(ex->plan.nodes[st0.srcB]);
      int64_t rbP = schemaRowBytes(ex->plan.nodes[st0.srcP]);
      int64_t nB = bindingRows(ex, st0.srcB);
      int64_t nP = bindingRows(ex, st0.srcP);
      int64_t need = nB * rbB + nP * rbP + nP * (rbB + rbP);
      int64_t budget = hbmBudgetBytes();
      if (need > budget) {
        int nParts = (int)std::min<int64_t>(
            256, std::max<int64_t>(2, need * 2 / std::max<int64_t>(budget, 1)));
        int64_t sliceRows = std::max<int64_t>(
            1024, budget / 4 / std::max<int64_t>(rbB + rbP, 1));
        int32_t rc = partitionJoinSide(ex, st0, 0, nParts, sliceRows,
                                       &ex->spillB);
        if (rc == GX_OK)
          rc = partitionJoinSide(ex, st0, 1, nParts, sliceRows, &ex->spillP);
        if (rc) return rc;
        ex->joinSpill = true;
        ex->joinSpillMark = ex->devBufs.size();
        if (getenv("GX_DEBUG"))
          fprintf(stderr, "[gx] join spill: %d partitions (need %lld > budget %lld)\n",
                  nParts, (long long)need, (long long)budget);
      }
    }
    if (ex->joinSpill) {
      ex->joinSpillCur = -1;
      ex->joinSpillMatches = 0;
      return joinSpillAdvance(ex);
    }
  }
  // persistent per-stage state (counters + cached source materializations)
  // is allocated before the per-run scope opens
  for (size_t s = 0; s < ex->joinStages.size(); s++) {
    gx_exec::JoinStage& st = ex->joinStages[s];
    if (!st.hj.counters) {
      st.hj.counters = (uint64_t*)devAllocP(ex, 3 * 8);
      if (!st.hj.counters) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    }
    if (!st.inputsReady) {
      if (st.srcB >= 0) {
        int32_t rc = materializeTable(ex, st.srcB, &st.buildTab);
        if (rc) return rc;
      }
      if (st.srcP >= 0) {
        int32_t rc = materializeTable(ex, st.srcP, &st.probeTab);
        if (rc) return rc;
      }
      st.inputsReady = true;
    }
  }
  beginRun(ex);
  for (size_t s = 0; s < ex->joinStages.size(); s++) {
    gx_exec::JoinStage& st = ex->joinStages[s];
    st.hj.errorFlag = ex->devErr;
    int32_t rc = runJoinStage(ex, st, s + 1 == ex->joinStages.size());
    if (rc) return rc;
  }
  // root stage output becomes the engine's resident table (emission / sort /
  // fused aggregation all read desc.table)
  gx_exec::JoinStage& root = ex->joinStages.back();
  for (int c = 0; c < root.out.nCols; c++)
    ex->desc.table.cols[c] = root.out.cols[c];
  ex->desc.table.nCols = root.out.nCols;
  ex->desc.table.nRows = root.out.nRows;
  ex->srcPos = 0;
  return GX_OK;
}

// ---------------- standalone selection execution ----------------

static int32_t runSelect(gx_exec* ex) {
  gx_exec::JoinStage& st = ex->selStage;
  gxp::HashJoinDesc& hj = st.hj;
  if (!ex->deviceReady) {
    if (!gpuAvailable()) {
      ex->err = "no MI355X visible: the product engine has no CPU fallback "
                "(GX_ERR_NO_GPU)";
      return GX_ERR_NO_GPU;
    }
    if (ex->device >= 0) hipSetDevice(ex->device);
    HIP_OK(ex, hipStreamCreate(&ex->stream));
    ex->devErr = (uint32_t*)devAllocP(ex, 4);
    ex->devHj = (gxp::HashJoinDesc*)devAllocP(ex, sizeof(gxp::HashJoinDesc));
    hj.counters = (uint64_t*)devAllocP(ex, 3 * 8);
    if (!ex->devErr || !ex->devHj || !hj.counters) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
    hj.errorFlag = ex->devErr;
    int32_t rc = materializeTable(ex, st.srcP, &st.probeTab);
    if (rc) return rc;
    ex->deviceReady = true;
  }
  beginRun(ex);
  hj.probe = st.probeTab;
  if (hj.probe.nRows > 0xFFFFFFFFLL) {
    ex->err = "selection > 2^32 rows unsupported this round";
    return GX_ERR_INVALID;
  }
  hipEvent_t ev0, ev1;
  HIP_OK(ex, hipEventCreate(&ev0));
  HIP_OK(ex, hipEventCreate(&ev1));
  HIP_OK(ex, hipEventRecord(ev0, ex->stream));
  HIP_OK(ex, hipMemsetAsync(hj.counters, 0, 24, ex->stream));
  HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
  HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj), hipMemcpyHostToDevice,
                            ex->stream));
  if (gxp::gxSelectPhase(0, ex->devHj, hj, ex->stream) != 0) {
    ex->err = "selection kernel launch failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  uint64_t total = 0;
  HIP_OK(ex, hipMemcpy(&total, hj.counters, 8, hipMemcpyDeviceToHost));
  setTableMeta(&st.out, st.types, st.fracs);
  st.out.nRows = 0;
  if (total > 0) {
    hj.outProbe = (uint32_t*)devAlloc(ex, total * 4);
    if (!hj.outProbe) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    HIP_OK(ex, hipMemcpyAsync(ex->devHj, &hj, sizeof(hj),
                              hipMemcpyHostToDevice, ex->stream));
    if (gxp::gxSelectPhase(1, ex->devHj, hj, ex->stream) != 0) {
      ex->err = "selection fill launch failed";
      return GX_ERR_INTERNAL;
    }
    // restore input row order (SelectionExec appends survivors in order;
    // the wave-aggregated compaction is order-free)
    uint32_t* sorted = (uint32_t*)devAlloc(ex, total * 4);
    size_t tmpBytes = 0;
    gxp::gxSortU32Keys(hj.outProbe, sorted, (int64_t)total, nullptr,
                       &tmpBytes, ex->stream);
    void* tmp = devAlloc(ex, std::max<size_t>(tmpBytes, 1));
    if (!sorted || !tmp) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
    if (gxp::gxSortU32Keys(hj.outProbe, sorted, (int64_t)total, tmp,
                           &tmpBytes, ex->stream) != 0) {
      ex->err = "selection index sort failed";
      return GX_ERR_INTERNAL;
    }
    int32_t rc = gatherCols(ex, hj.probe, sorted, total, &st.out, 0);
    if (rc) return rc;
  }
  HIP_OK(ex, hipEventRecord(ev1, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  {
    float ms = 0;
    hipEventElapsedTime(&ms, ev0, ev1);
    ex->lastKernelMs = ms;
    hipEventDestroy(ev0);
    hipEventDestroy(ev1);
  }
  ex->lastSelCount = total;
  st.out.nRows = (int64_t)total;
  for (int c = 0; c < st.out.nCols; c++)
    ex->desc.table.cols[c] = st.out.cols[c];
  ex->desc.table.nRows = st.out.nRows;
  ex->srcPos = 0;
  return GX_OK;
}

// ---------------- standalone projection execution ----------------

// bytes of a ProjDesc the device reads: the composed string programs come
// last, and the upload ends after the ones in use
static size_t projDescUploadBytes(const gxp::ProjDesc& h) {
  return offsetof(gxp::ProjDesc, cat) +
         (size_t)h.nCat * sizeof(gxp::StrCatProg);
}

static int32_t runProject(gx_exec* ex) {
  gxp::ProjDesc& pd = ex->pd;
  if (!ex->projOverSelect) ex->lastKernelMs = 0;  // else runSelect seeds it
  if (ex->projOverSelect) {
    // materialize the filtered input first (runSelect leaves its output in
    // selStage.out and clobbers desc.table meta; we restore below)
    int32_t rc = runSelect(ex);
    if (rc) return rc;
    pd.table = ex->selStage.out;
  } else {
    if (!ex->deviceReady) {
      if (!gpuAvailable()) {
        ex->err = "no MI355X visible: the product engine has no CPU fallback "
                  "(GX_ERR_NO_GPU)";
        return GX_ERR_NO_GPU;
      }
      if (ex->device >= 0) hipSetDevice(ex->device);
      HIP_OK(ex, hipStreamCreate(&ex->stream));
      ex->devErr = (uint32_t*)devAllocP(ex, 4);
      if (!ex->devErr) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
      int32_t rc = materializeTable(ex, ex->projSrcNode, &ex->selStage.probeTab);
      if (rc) return rc;
      ex->deviceReady = true;
    }
    beginRun(ex);  // projOverSelect re-runs open the scope inside runSelect
    pd.table = ex->selStage.probeTab;
  }
  if (!ex->devPd) {
    ex->devPd = (gxp::ProjDesc*)devAllocP(ex, sizeof(gxp::ProjDesc));
    if (!ex->devPd) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  }
  pd.errorFlag = ex->devErr;
  int64_t n = pd.table.nRows;
  // computed-output buffers
  std::vector<uint8_t*> bitmaps(pd.nOut, nullptr);
  for (int o = 0; o < pd.nOut && n > 0; o++) {
    int es = pd.outType[o] == GX_TYPE_DECIMAL ? 40 : 8;
    pd.outData[o] = devAlloc(ex, (size_t)n * es);
    pd.outNotNull[o] = (uint8_t*)devAlloc(ex, (size_t)n);
    bitmaps[o] = (uint8_t*)devAlloc(ex, (n + 7) / 8);
    if (!pd.outData[o] || !pd.outNotNull[o] || !bitmaps[o]) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
  }
  // string-program temps + outputs (allocated before the devPd upload and
  // OUTSIDE the timed window; output bytes are bounded by the source
  // column's bytes — windows only shrink)
  std::vector<int64_t*> spOffsets(pd.nSprog, nullptr);
  std::vector<void*> spData(pd.nSprog, nullptr);
  std::vector<uint8_t*> spBitmaps(pd.nSprog, nullptr);
  std::vector<void*> spTmp(pd.nSprog, nullptr);
  std::vector<size_t> spTmpBytes(pd.nSprog, 0);
  for (int si = 0; si < pd.nSprog && n > 0; si++) {
    gxp::StrProg& sp = pd.sprog[si];
    sp.starts = (int64_t*)devAlloc(ex, (size_t)n * 8);
    sp.lens = (int64_t*)devAlloc(ex, (size_t)n * 8);
    sp.notNull = (uint8_t*)devAlloc(ex, (size_t)n);
    spOffsets[si] = (int64_t*)devAlloc(ex, ((size_t)n + 1) * 8);
    spBitmaps[si] = (uint8_t*)devAlloc(ex, (n + 7) / 8);
    const gxp::DevCol& srcc = pd.table.cols[sp.col];
    int64_t srcBytes = (int64_t)n;  // dense char(1)
    if (!srcc.denseOffsets && srcc.offsets) {
      HIP_OK(ex, hipMemcpy(&srcBytes, srcc.offsets + n, 8,
                           hipMemcpyDeviceToHost));
    }
    spData[si] = devAlloc(ex, std::max<int64_t>(srcBytes, 1) + 16);
    gxp::gxExclusiveSumI64(sp.lens, spOffsets[si], n, nullptr,
                           &spTmpBytes[si], ex->stream);
    spTmp[si] = devAlloc(ex, std::max<size_t>(spTmpBytes[si], 1));
    if (!sp.starts || !sp.lens || !sp.notNull || !spOffsets[si] ||
        !spBitmaps[si] || !spData[si] || !spTmp[si]) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
  }
  // composed string programs: 9 B/row of lens + notNull, the offsets, and
  // an output buffer sized from an upper bound computed in int64_t (a window
  // never exceeds its column's bytes, an integer's text is <= 20 bytes), so
  // nothing is read back inside the timed window
  struct CatBufs {
    int64_t* lens = nullptr;
    uint8_t* notNull = nullptr;
    int64_t* offsets = nullptr;
    uint8_t* bitmap = nullptr;
    void* data = nullptr;
    void* tmp = nullptr;
    size_t tmpBytes = 0;
  };
  std::vector<CatBufs> cat(pd.nCat);
  std::map<int, int64_t> colBytes;  // string column -> total bytes
  for (int ci = 0; ci < pd.nCat && n > 0; ci++) {
    const gxp::StrCatProg& cp = pd.cat[ci];
    int64_t bound = cp.ws ? n * (int64_t)(cp.nPieces - 1) * cp.sepLen : 0;
    for (int p = 0; p < cp.nPieces; p++) {
      const gxp::StrPiece& pc = cp.piece[p];
      if (pc.kind == gxp::SPK_CONST) {
        bound += n * (int64_t)pc.constLen;
      } else if (pc.kind == gxp::SPK_I64) {
        bound += n * 20;
      } else {
        auto it = colBytes.find(pc.col);
        if (it == colBytes.end()) {
          const gxp::DevCol& srcc = pd.table.cols[pc.col];
          int64_t srcBytes = n;  // dense char(1)
          if (!srcc.denseOffsets && srcc.offsets)
            HIP_OK(ex, hipMemcpy(&srcBytes, srcc.offsets + n, 8,
                                 hipMemcpyDeviceToHost));
          it = colBytes.emplace(pc.col, srcBytes).first;
        }
        bound += it->second;
      }
    }
    CatBufs& cb = cat[ci];
    cb.lens = (int64_t*)devAlloc(ex, (size_t)n * 8);
    cb.notNull = (uint8_t*)devAlloc(ex, (size_t)n);
    cb.offsets = (int64_t*)devAlloc(ex, ((size_t)n + 1) * 8);
    cb.bitmap = (uint8_t*)devAlloc(ex, (n + 7) / 8);
    cb.data = devAlloc(ex, (size_t)std::max<int64_t>(bound, 1));
    gxp::gxExclusiveSumI64(cb.lens, cb.offsets, n, nullptr, &cb.tmpBytes,
                           ex->stream);
    cb.tmp = devAlloc(ex, std::max<size_t>(cb.tmpBytes, 1));
    if (!cb.lens || !cb.notNull || !cb.offsets || !cb.bitmap || !cb.data ||
        !cb.tmp) {
      ex->err = "hipMalloc failed";
      return GX_ERR_INTERNAL;
    }
  }
  // the timed window covers the kernels, not the multi-GB hipMalloc churn
  hipEvent_t ev0, ev1;
  HIP_OK(ex, hipEventCreate(&ev0));
  HIP_OK(ex, hipEventCreate(&ev1));
  HIP_OK(ex, hipEventRecord(ev0, ex->stream));
  for (int attempt = 0; n > 0 && attempt < 2; attempt++) {
    HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
    HIP_OK(ex, hipMemcpyAsync(ex->devPd, &pd, projDescUploadBytes(pd),
                              hipMemcpyHostToDevice, ex->stream));
    if (gxp::gxProject(ex->devPd, pd, ex->stream) != 0) {
      ex->err = "projection kernel launch failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    uint32_t errFlag = 0;
    HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
    if (errFlag == 256u /*kErrRetryWide*/ && !pd.wide) {
      pd.wide = 1;  // int64 fast path overflowed: rerun with the int128 VM
      continue;
    }
    errFlag &= ~256u;
    if (errFlag != 0) {
      ex->err = "device projection error flag 0x" + std::to_string(errFlag);
      return GX_ERR_INTERNAL;
    }
    break;
  }
  for (int o = 0; o < pd.nOut && n > 0; o++) {
    if (gxp::gxPackNulls(pd.outNotNull[o], bitmaps[o], n, ex->stream) != 0) {
      ex->err = "null pack launch failed";
      return GX_ERR_INTERNAL;
    }
  }
  // string programs: window views -> scanned offsets -> byte emit (buffers
  // pre-allocated above; no sync inside)
  for (int si = 0; si < pd.nSprog && n > 0; si++) {
    gxp::StrProg& sp = pd.sprog[si];
    if (gxp::gxStrWindow(ex->devPd, pd, si, ex->stream) != 0) {
      ex->err = "string window launch failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipMemsetAsync(spOffsets[si], 0, 8, ex->stream));
    if (gxp::gxExclusiveSumI64(sp.lens, spOffsets[si], n, spTmp[si],
                               &spTmpBytes[si], ex->stream) != 0) {
      ex->err = "string offsets scan failed";
      return GX_ERR_INTERNAL;
    }
    if (gxp::gxStrEmit(ex->devPd, pd, si, spOffsets[si],
                       (uint8_t*)spData[si], ex->stream) != 0 ||
        gxp::gxPackNulls(sp.notNull, spBitmaps[si], n, ex->stream) != 0) {
      ex->err = "string emit launch failed";
      return GX_ERR_INTERNAL;
    }
  }
  // composed string programs: row lengths -> scanned offsets -> tile emit
  // (hidden integer arguments were written by the projection kernel above)
  for (int ci = 0; ci < pd.nCat && n > 0; ci++) {
    CatBufs& cb = cat[ci];
    if (gxp::gxStrCatLens(ex->devPd, pd, ci, cb.lens, cb.notNull,
                          ex->stream) != 0) {
      ex->err = "composed string length launch failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipMemsetAsync(cb.offsets, 0, 8, ex->stream));
    if (gxp::gxExclusiveSumI64(cb.lens, cb.offsets, n, cb.tmp, &cb.tmpBytes,
                               ex->stream) != 0) {
      ex->err = "string offsets scan failed";
      return GX_ERR_INTERNAL;
    }
    if (gxp::gxStrCatEmit(ex->devPd, pd, ci, cb.offsets, (uint8_t*)cb.data,
                          ex->stream) != 0 ||
        gxp::gxPackNulls(cb.notNull, cb.bitmap, n, ex->stream) != 0) {
      ex->err = "composed string emit launch failed";
      return GX_ERR_INTERNAL;
    }
  }
  HIP_OK(ex, hipEventRecord(ev1, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  {
    float ms = 0;
    hipEventElapsedTime(&ms, ev0, ev1);
    ex->lastKernelMs += ms;
    hipEventDestroy(ev0);
    hipEventDestroy(ev1);
  }
  if (pd.nCat > 0 && n > 0) {
    uint32_t errFlag = 0;
    HIP_OK(ex, hipMemcpy(&errFlag, ex->devErr, 4, hipMemcpyDeviceToHost));
    if (errFlag & 512u /*kErrStrRowTooLong*/) {
      ex->err = "a CONCAT / CONCAT_WS output row exceeds 2 GiB";
      return GX_ERR_INVALID;
    }
  }
  // assemble the output table: passthrough columns alias the input buffers
  ex->desc.table.nCols = (int)ex->projOutTypes.size();
  for (size_t c = 0; c < ex->projOutTypes.size(); c++) {
    gxp::DevCol& dst = ex->desc.table.cols[c];
    if (ex->projOutSrcCol[c] >= 0) {
      dst = pd.table.cols[ex->projOutSrcCol[c]];
    } else if (ex->projOutSprog[c] >= 0) {
      int si = ex->projOutSprog[c];
      setDevColMeta(&dst, GX_TYPE_STRING, 0);
      dst.data = n > 0 ? spData[si] : nullptr;
      dst.offsets = n > 0 ? spOffsets[si] : nullptr;
      dst.nullBitmap = n > 0 ? spBitmaps[si] : nullptr;
      dst.hasNulls = n > 0 ? 1 : 0;
      dst.denseOffsets = 0;
    } else if (ex->projOutCat[c] >= 0) {
      const CatBufs& cb = cat[ex->projOutCat[c]];
      setDevColMeta(&dst, GX_TYPE_STRING, 0);
      dst.data = cb.data;
      dst.offsets = cb.offsets;
      dst.nullBitmap = cb.bitmap;
      dst.hasNulls = n > 0 ? 1 : 0;
      dst.denseOffsets = 0;
    } else {
      int o = ex->projOutSlot[c];
      setDevColMeta(&dst, ex->projOutTypes[c], ex->projOutFracs[c]);
      dst.data = pd.outData[o];
      dst.offsets = nullptr;
      dst.nullBitmap = n > 0 ? bitmaps[o] : nullptr;
      dst.hasNulls = n > 0 ? 1 : 0;
      dst.denseOffsets = 0;
    }
  }
  ex->desc.table.nRows = n;
  ex->lastSelCount = (uint64_t)n;
  ex->srcPos = 0;
  return GX_OK;
}

// ---------------- FINAL-mode host merge ----------------

static int32_t runFinalHost(gx_exec* ex) {
  const PNode& agg = ex->plan.nodes[ex->root];
  auto it = ex->bindings.find(agg.child);
  if (it == ex->bindings.end() || !it->second.haveChunks) {
    ex->err = "FINAL mode needs bound partial chunks";
    return GX_ERR_INVALID;
  }
  gxp::FinalSpec spec;
  spec.nGroup = agg.exprs.size();
  spec.funcs = agg.aggFuncs;
  spec.fracs = agg.aggFracs;
  for (int argE : agg.aggArgs)
    spec.argIsF64.push_back(argE >= 0 &&
                            ex->plan.exprs[argE].retType == GX_TYPE_F64);
  return gxp::mergeFinal(it->second.chunks, spec, &ex->resultRows, &ex->err);
}

// ---------------- bare source download (generator parity) ----------------

// scratch the device sort owns before its LSD chain starts; the string rank
// build borrows it
struct SortScratch {
  uint32_t *idxA, *idxB;
  uint64_t *keyA, *keyB;
  uint64_t* devOrAnd;
  void* tmp;
  size_t tmpBytes;
};

// a hipcub temp buffer of at least `need` bytes: the sort's own when it is
// large enough, else a new allocation that replaces it
static void* sortTmpFor(gx_exec* ex, SortScratch& sc, size_t need) {
  if (need > sc.tmpBytes) {
    void* t = devAlloc(ex, need);
    if (!t) return nullptr;
    sc.tmp = t;
    sc.tmpBytes = need;
  }
  return sc.tmp;
}

// dense order rank of a general varlen column (gx_strkey.h): rank[a] <
// rank[b] iff row a's string orders before row b's under utf8mb4_bin PAD
// SPACE, equal iff they compare equal; NULL rows rank with the empty string
// (the chain's null-bit pass places them). MSD refinement over 7-byte window
// keys: each round sorts only the rows whose prefix is still shared, inside
// their tied position ranges. *rankOut stays allocated; the scratch is freed.
static int32_t buildStringRank(gx_exec* ex, const gxp::DevCol& col, int64_t n,
                               SortScratch& sc, uint32_t** rankOut) {
  if (n > 0x7FFFFFFFLL) {
    ex->err = "string sort key over > 2^31 rows unsupported";
    return GX_ERR_INVALID;
  }
  uint32_t* rank = (uint32_t*)devAlloc(ex, n * 4);
  if (!rank) { ex->err = "hipMalloc failed (string rank)"; return GX_ERR_INTERNAL; }
  const size_t mark = ex->devBufs.size();
  uint32_t* elen = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* perm = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* head = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* rowAct = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* seg = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* hflag = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* iota = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* actA = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* actB = (uint32_t*)devAlloc(ex, n * 4);
  uint64_t* wSorted = (uint64_t*)devAlloc(ex, n * 8);
  uint8_t* keep = (uint8_t*)devAlloc(ex, n);
  uint32_t* devWord = (uint32_t*)devAlloc(ex, 8);  // [0] max elen / count
  if (!elen || !perm || !head || !rowAct || !seg || !hflag || !iota || !actA ||
      !actB || !wSorted || !keep || !devWord) {
    ex->err = "hipMalloc failed (string rank)";
    return GX_ERR_INTERNAL;
  }
  size_t scanBytes = 0, selBytes = 0;
  gxp::gxInclusiveSumU32(hflag, seg, n, nullptr, &scanBytes, ex->stream);
  gxp::gxSelectFlaggedU32(nullptr, keep, actA, devWord, n, nullptr, &selBytes,
                          ex->stream);
  if (!sortTmpFor(ex, sc, std::max(scanBytes, selBytes))) {
    ex->err = "hipMalloc failed (string rank)";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipMemsetAsync(devWord, 0, 8, ex->stream));
  HIP_OK(ex, hipMemsetAsync(head, 0, n * 4, ex->stream));
  if (gxp::gxSortIota(iota, n, ex->stream) ||
      gxp::gxStrKeyElen(col, n, elen, devWord, ex->devErr, ex->stream)) {
    ex->err = "string rank launch failed";
    return GX_ERR_INTERNAL;
  }
  uint32_t hw[2] = {0, 0};
  HIP_OK(ex, hipMemcpyAsync(hw, devWord, 4, hipMemcpyDeviceToHost, ex->stream));
  HIP_OK(ex, hipMemcpyAsync(hw + 1, ex->devErr, 4, hipMemcpyDeviceToHost,
                            ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  if (hw[1] & 512u) {  // kErrStrRowTooLong
    ex->err = "string sort key longer than 2^32-1 bytes";
    return GX_ERR_INVALID;
  }
  // the loop is bounded on the host: a row is active in round r > 0 only if
  // its effective length reaches 7r
  const uint32_t maxRounds = gxp::strKeyMaxRounds(hw[0]);
  const uint32_t* act = nullptr;  // round 0: position i, row i
  uint32_t* actNext = actA;
  int64_t m = n;
  uint32_t round = 0;
  while (m > 0) {
    if (round >= maxRounds) {
      ex->err = "internal: string rank refinement ran past its round bound";
      return GX_ERR_INTERNAL;
    }
    uint64_t* w = sc.keyA;
    if (gxp::gxStrKeyCompose(col, elen, perm, act, head, m, round, w, rowAct,
                             hflag, ex->stream) ||
        gxp::gxSortKeyBits(w, m, sc.devOrAnd, ex->stream)) {
      ex->err = "string rank launch failed";
      return GX_ERR_INTERNAL;
    }
    size_t tb = sc.tmpBytes;
    if (gxp::gxInclusiveSumU32(hflag, seg, m, sc.tmp, &tb, ex->stream)) {
      ex->err = "string rank segment scan failed";
      return GX_ERR_INTERNAL;
    }
    uint64_t oa[2];
    uint32_t nSeg = 0;
    HIP_OK(ex, hipMemcpyAsync(oa, sc.devOrAnd, 16, hipMemcpyDeviceToHost,
                              ex->stream));
    HIP_OK(ex, hipMemcpyAsync(&nSeg, seg + (m - 1), 4, hipMemcpyDeviceToHost,
                              ex->stream));
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    // order[j] = the active slot whose row stands at slot j afterwards
    const uint32_t* order = nullptr;
    uint64_t diff = oa[0] ^ oa[1];
    if (diff != 0) {
      int beginBit = __builtin_ctzll(diff);
      int endBit = 64 - __builtin_clzll(diff);
      if (endBit == 64) beginBit = 0;  // rocPRIM mask overflow, see below
      size_t need = 0;
      gxp::gxSortPairs(w, sc.keyB, iota, sc.idxA, m, nullptr, &need, beginBit,
                       endBit, ex->stream);
      if (!sortTmpFor(ex, sc, need)) {
        ex->err = "hipMalloc failed (string rank)";
        return GX_ERR_INTERNAL;
      }
      size_t tb1 = sc.tmpBytes;
      if (gxp::gxSortPairs(w, sc.keyB, iota, sc.idxA, m, sc.tmp, &tb1,
                           beginBit, endBit, ex->stream)) {
        ex->err = "string rank window sort failed";
        return GX_ERR_INTERNAL;
      }
      order = sc.idxA;
      if (nSeg > 1) {
        // stable by segment id (1..nSeg): rows return to their own tied
        // range, in window order inside it
        int segEnd = 64 - __builtin_clzll((uint64_t)nSeg);
        uint64_t* segKeys = sc.keyB;  // the sorted windows are not needed
        if (gxp::gxStrKeySegKeys(seg, sc.idxA, segKeys, m, ex->stream)) {
          ex->err = "string rank launch failed";
          return GX_ERR_INTERNAL;
        }
        need = 0;
        gxp::gxSortPairs(segKeys, wSorted, sc.idxA, sc.idxB, m, nullptr, &need,
                         0, segEnd, ex->stream);
        if (!sortTmpFor(ex, sc, need)) {
          ex->err = "hipMalloc failed (string rank)";
          return GX_ERR_INTERNAL;
        }
        size_t tb2 = sc.tmpBytes;
        if (gxp::gxSortPairs(segKeys, wSorted, sc.idxA, sc.idxB, m, sc.tmp,
                             &tb2, 0, segEnd, ex->stream)) {
          ex->err = "string rank segment sort failed";
          return GX_ERR_INTERNAL;
        }
        order = sc.idxB;
      }
    }
    size_t tb3 = sc.tmpBytes;
    if (gxp::gxStrKeyPlace(w, rowAct, order, act, perm, wSorted, m,
                           ex->stream) ||
        gxp::gxStrKeyRefine(seg, wSorted, act, head, keep, m, ex->stream) ||
        gxp::gxSelectFlaggedU32(act, keep, actNext, devWord, m, sc.tmp, &tb3,
                                ex->stream)) {
      ex->err = "string rank launch failed";
      return GX_ERR_INTERNAL;
    }
    uint32_t kept = 0;
    HIP_OK(ex, hipMemcpyAsync(&kept, devWord, 4, hipMemcpyDeviceToHost,
                              ex->stream));
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    if ((int64_t)kept > m) {
      ex->err = "internal: string rank active set grew";
      return GX_ERR_INTERNAL;
    }
    m = kept;
    act = actNext;
    actNext = actNext == actA ? actB : actA;
    round++;
  }
  size_t tb4 = sc.tmpBytes;
  if (gxp::gxInclusiveSumU32(head, seg, n, sc.tmp, &tb4, ex->stream) ||
      gxp::gxStrKeyScatterRank(perm, seg, rank, n, ex->stream)) {
    ex->err = "string rank launch failed";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  if (getenv("GX_DEBUG"))
    fprintf(stderr, "[gx] string rank: %lld rows, max effective length %u, "
            "%u refinement rounds\n", (long long)n, hw[0], round);
  // a larger tmp allocated above replaces the sort's own: it stays
  size_t from = mark;
  auto tmpAt = std::find(ex->devBufs.begin() + mark, ex->devBufs.end(), sc.tmp);
  if (tmpAt != ex->devBufs.end()) {
    std::iter_swap(ex->devBufs.begin() + mark, tmpAt);
    from = mark + 1;
  }
  freeSince(ex, from);
  *rankOut = rank;
  return GX_OK;
}

// run the device radix sort once, replacing the table's column buffers with
// gathered sorted copies (stable LSD passes, innermost key first)
static int32_t runDeviceSort(gx_exec* ex) {
  gxp::DevTable& tab = ex->desc.table;
  int64_t n = tab.nRows;
  if (n > 0xFFFFFFFFLL) { ex->err = "sort > 2^32 rows unsupported"; return GX_ERR_INVALID; }
  if (n == 0) { ex->devSorted = true; return GX_OK; }
  if (!ex->devErr) ex->devErr = (uint32_t*)devAllocP(ex, 4);
  if (!ex->devErr) { ex->err = "hipMalloc failed (sort err)"; return GX_ERR_INTERNAL; }
  uint32_t* idxA = (uint32_t*)devAlloc(ex, n * 4);
  uint32_t* idxB = (uint32_t*)devAlloc(ex, n * 4);
  uint64_t* keyA = (uint64_t*)devAlloc(ex, n * 8);
  uint64_t* keyB = (uint64_t*)devAlloc(ex, n * 8);
  uint64_t* devOrAnd = (uint64_t*)devAlloc(ex, 16);
  size_t tmpBytes = 0;
  gxp::gxSortPairs(keyA, keyB, idxA, idxB, n, nullptr, &tmpBytes, 0, 64,
                   ex->stream);
  void* tmp = devAlloc(ex, tmpBytes);
  if (!idxA || !idxB || !keyA || !keyB || !tmp) {
    ex->err = "hipMalloc failed (sort)";
    return GX_ERR_INTERNAL;
  }
  HIP_OK(ex, hipMemsetAsync(ex->devErr, 0, 4, ex->stream));
  hipEvent_t ev0, ev1;
  hipEventCreate(&ev0);
  hipEventCreate(&ev1);
  hipEventRecord(ev0, ex->stream);
  // a general varlen key becomes a dense rank column once, before the chain
  // (a dense char(1) key stays kind 2); the same column twice shares a rank
  std::vector<gxp::SortKeyCompose> sortKeys = ex->devSortKeys;
  for (size_t j = 0; j < sortKeys.size(); j++) {
    gxp::SortKeyCompose& k = sortKeys[j];
    if (k.kind != 2 || tab.cols[k.col].denseOffsets) continue;
    for (size_t i = 0; i < j && !k.rank; i++)
      if (sortKeys[i].kind == 4 && sortKeys[i].col == k.col)
        k.rank = sortKeys[i].rank;
    if (!k.rank) {
      SortScratch sc{idxA, idxB, keyA, keyB, devOrAnd, tmp, tmpBytes};
      uint32_t* rank = nullptr;
      int32_t rrc = buildStringRank(ex, tab.cols[k.col], n, sc, &rank);
      if (rrc != GX_OK) return rrc;
      tmp = sc.tmp;
      tmpBytes = sc.tmpBytes;
      k.rank = rank;
    }
    k.kind = 4;
  }
  if (gxp::gxSortIota(idxA, n, ex->stream)) { ex->err = "iota launch failed"; return GX_ERR_INTERNAL; }
  for (int j = (int)sortKeys.size() - 1; j >= 0; j--) {
    if (gxp::gxSortComposeKeys(nullptr, tab, sortKeys[j], idxA, keyA, n,
                               ex->devErr, ex->stream)) {
      ex->err = "key compose launch failed";
      return GX_ERR_INTERNAL;
    }
    // bound the radix to the bits that actually differ across keys
    uint64_t oa[2];
    if (gxp::gxSortKeyBits(keyA, n, devOrAnd, ex->stream)) {
      ex->err = "key bits launch failed";
      return GX_ERR_INTERNAL;
    }
    HIP_OK(ex, hipMemcpyAsync(oa, devOrAnd, 16, hipMemcpyDeviceToHost,
                              ex->stream));
    HIP_OK(ex, hipStreamSynchronize(ex->stream));
    uint64_t diff = oa[0] ^ oa[1];
    // all keys equal -> the value pass is skippable, but a nullable column
    // still needs its null-bit pass below
    if (diff != 0) {
      int beginBit = __builtin_ctzll(diff);
      int endBit = 64 - __builtin_clzll(diff);
      // rocPRIM's merge-sort path (1024 < n <= its merge limit) compares
      // keys under a mask built as (1 << end_bit) - 1, which shifts a
      // 64-bit one by 64 when end_bit is 64 and begin_bit is not 0: the
      // mask degenerates and the rows come out ordered by their low bits.
      // With begin_bit 0 it takes the unmasked compare. (Keys that reach
      // bit 63 and share their low bits: even int64 of both signs.)
      if (endBit == 64) beginBit = 0;
      size_t tb = tmpBytes;
      if (gxp::gxSortPairs(keyA, keyB, idxA, idxB, n, tmp, &tb, beginBit,
                           endBit, ex->stream)) {
        ex->err = "radix sort failed";
        return GX_ERR_INTERNAL;
      }
      std::swap(idxA, idxB);
    }
    // nullable key: a 1-bit stable pass ABOVE the value bits (sortexec
    // compare semantics: NULL < any value — first on ASC, last on DESC)
    const gxp::DevCol& kc = tab.cols[sortKeys[j].col];
    if (kc.hasNulls && kc.nullBitmap) {
      if (gxp::gxSortComposeNullKeys(kc.nullBitmap, idxA, keyA, n,
                                     sortKeys[j].desc, ex->stream)) {
        ex->err = "null key compose failed";
        return GX_ERR_INTERNAL;
      }
      size_t tb2 = tmpBytes;
      if (gxp::gxSortPairs(keyA, keyB, idxA, idxB, n, tmp, &tb2, 0, 1,
                           ex->stream)) {
        ex->err = "null radix pass failed";
        return GX_ERR_INTERNAL;
      }
      std::swap(idxA, idxB);
    }
  }
  uint32_t herr = 0;
  HIP_OK(ex, hipMemcpyAsync(&herr, ex->devErr, 4, hipMemcpyDeviceToHost, ex->stream));
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  if (herr) { ex->err = "sort key error (bad/overflowing decimal)"; return GX_ERR_INVALID; }
  // gather every column through the final permutation in ONE launch
  // (per-column kernels serialize on the stream; the random-access gather
  // is latency-bound and wants all columns' requests in flight together)
  {
    const void* ins[16];
    void* outs[16];
    int sizes[16];
    int nc = tab.nCols;
    if (nc > 16) { ex->err = "sort supports <= 16 columns this round"; return GX_ERR_INVALID; }
    for (int c = 0; c < nc; c++) {
      gxp::DevCol& col = tab.cols[c];
      // general varlen columns take the two-pass gather below
      if (col.type == GX_TYPE_STRING && !col.denseOffsets) {
        sizes[c] = 0;
        continue;
      }
      int es = col.type == GX_TYPE_DECIMAL ? 40
               : (col.type == GX_TYPE_STRING ? 1 : 8);
      void* nd = devAlloc(ex, (size_t)n * es + 16);
      if (!nd) { ex->err = "hipMalloc failed (gather)"; return GX_ERR_INTERNAL; }
      ins[c] = col.data;
      outs[c] = nd;
      sizes[c] = es;
    }
    // sequential per-column gathers measured FASTER than both a combined
    // single kernel and per-column concurrent streams: one column's random
    // reads stay L2-coherent; concurrent columns evict each other
    int grc = 0;
    for (int c = 0; c < nc; c++)
      if (sizes[c])
        grc |= gxp::gxSortGatherCol(ins[c], outs[c], idxA, n, sizes[c],
                                    ex->stream);
    // null bitmaps ride the same permutation (joined-table sort; generator
    // sources have none)
    for (int c = 0; c < nc; c++) {
      gxp::DevCol& col = tab.cols[c];
      if (col.hasNulls && col.nullBitmap) {
        uint8_t* nb = (uint8_t*)devAlloc(ex, (n + 7) / 8);
        if (!nb) { ex->err = "hipMalloc failed (null gather)"; return GX_ERR_INTERNAL; }
        grc |= gxp::gxGatherNulls(col.nullBitmap, idxA, nb, n, ex->stream);
        col.nullBitmap = nb;
      }
    }
    if (grc) {
      ex->err = "gather launch failed";
      return GX_ERR_INTERNAL;
    }
    for (int c = 0; c < nc; c++) {
      gxp::DevCol& col = tab.cols[c];
      if (sizes[c]) {
        col.data = outs[c];  // dense-char offsets stay the identity ramp
        continue;
      }
      gxp::DevCol nd = col;
      int32_t vrc = gatherVarlenCol(ex, col, idxA, (uint64_t)n, nd);
      if (vrc) return vrc;
      col.data = nd.data;
      col.offsets = nd.offsets;
    }
  }
  hipEventRecord(ev1, ex->stream);
  HIP_OK(ex, hipStreamSynchronize(ex->stream));
  float ms = 0;
  hipEventElapsedTime(&ms, ev0, ev1);
  ex->lastKernelMs = ms;
  hipEventDestroy(ev0);
  hipEventDestroy(ev1);
  ex->devSorted = true;
  // offset/limit: serve the slice [offset, offset+limit)
  ex->srcPos = ex->sliceStart = std::min<int64_t>(ex->devSortOffset, n);
  if (ex->devSortLimit >= 0)
    tab.nRows = std::min<int64_t>(n, ex->srcPos + ex->devSortLimit);
  return GX_OK;
}

// ---------------- out-of-core sort (spill runs + k-way merge) ----------------

// sort a source larger than the HBM budget: materialize + device-radix-sort
// row-range runs, download each sorted run (columns + composed order keys)
// to host, free the device buffers, then k-way merge on emission.
static int32_t runDeviceSortSpill(gx_exec* ex, int64_t runRows) {
  if (!gpuAvailable()) {
    ex->err = "no MI355X visible: the product engine has no CPU fallback "
              "(GX_ERR_NO_GPU)";
    return GX_ERR_NO_GPU;
  }
  if (ex->device >= 0) hipSetDevice(ex->device);
  if (!ex->stream) HIP_OK(ex, hipStreamCreate(&ex->stream));
  if (!ex->devErr) {
    ex->devErr = (uint32_t*)devAllocP(ex, 4);
    if (!ex->devErr) { ex->err = "hipMalloc failed"; return GX_ERR_INTERNAL; }
  }
  Binding& b = ex->bindings[ex->sourceNode];
  const int64_t total = b.tpchRows;
  const int64_t saveOffB = b.tpchRowOffset;
  const int64_t saveTotB = b.tpchTotalRows > 0 ? b.tpchTotalRows : total;
  gxp::DevTable saveTab = ex->desc.table;
  const int64_t saveLim = ex->devSortLimit, saveOff = ex->devSortOffset;
  const int nk = (int)ex->devSortKeys.size();
  const int ncols = saveTab.nCols;
  double sumMs = 0;
  int32_t rc = GX_OK;
  for (int64_t start = 0; start < total && rc == GX_OK; start += runRows) {
    int64_t n = std::min(runRows, total - start);
    size_t mark = ex->devBufs.size();
    b.tpchRowOffset = saveOffB + start;
    b.tpchRows = n;
    b.tpchTotalRows = saveTotB;
    gxp::DevTable runTab{};
    rc = materializeTable(ex, ex->sourceNode, &runTab);
    if (rc == GX_OK) {
      for (int c = 0; c < runTab.nCols && rc == GX_OK; c++) {
        if (runTab.cols[c].type == GX_TYPE_STRING &&
            !runTab.cols[c].denseOffsets) {
          ex->err = "general varlen column in spill sort unsupported this round";
          rc = GX_ERR_INVALID;
        }
        // emitSpillChunk emits all-NOT-NULL bitmaps; a nullable source would
        // silently lose its NULL flags — reject instead
        if (runTab.cols[c].hasNulls && runTab.cols[c].nullBitmap) {
          ex->err = "nullable column in spill sort unsupported this round";
          rc = GX_ERR_INVALID;
        }
      }
    }
    if (rc == GX_OK) {
      ex->desc.table = runTab;
      ex->devSortLimit = -1;
      ex->devSortOffset = 0;
      ex->devSorted = false;
      rc = runDeviceSort(ex);
      sumMs += ex->lastKernelMs;
    }
    if (rc == GX_OK) {
      // download the sorted run + its composed order keys
      gxp::DevTable& st = ex->desc.table;
      SortRun run;
      run.n = n;
      run.colData.resize(ncols);
      run.keys.resize(nk);
      uint32_t* iden = (uint32_t*)devAlloc(ex, n * 4);
      uint64_t* kbuf = (uint64_t*)devAlloc(ex, n * 8);
      if (!iden || !kbuf) { ex->err = "hipMalloc failed"; rc = GX_ERR_INTERNAL; }
      if (rc == GX_OK && gxp::gxSortIota(iden, n, ex->stream) != 0) {
        ex->err = "iota launch failed";
        rc = GX_ERR_INTERNAL;
      }
      for (int j = 0; j < nk && rc == GX_OK; j++) {
        if (gxp::gxSortComposeKeys(nullptr, st, ex->devSortKeys[j], iden,
                                   kbuf, n, ex->devErr, ex->stream) != 0) {
          ex->err = "key compose launch failed";
          rc = GX_ERR_INTERNAL;
          break;
        }
        run.keys[j].resize(n);
        if (hipMemcpy(run.keys[j].data(), kbuf, n * 8,
                      hipMemcpyDeviceToHost) != hipSuccess) {
          ex->err = "key download failed";
          rc = GX_ERR_INTERNAL;
        }
      }
      for (int c = 0; c < ncols && rc == GX_OK; c++) {
        const gxp::DevCol& col = st.cols[c];
        int es = col.type == GX_TYPE_DECIMAL ? 40
                 : (col.type == GX_TYPE_STRING ? 1 : 8);
        run.colData[c].resize((size_t)n * es);
        if (hipMemcpy(run.colData[c].data(), col.data, (size_t)n * es,
                      hipMemcpyDeviceToHost) != hipSuccess) {
          ex->err = "run download failed";
          rc = GX_ERR_INTERNAL;
        }
      }
      if (rc == GX_OK) ex->sortRuns.push_back(std::move(run));
    }
    freeSince(ex, mark);
  }
  b.tpchRowOffset = saveOffB;
  b.tpchRows = total;
  b.tpchTotalRows = saveTotB;
  ex->desc.table = saveTab;
  ex->devSortLimit = saveLim;
  ex->devSortOffset = saveOff;
  ex->devSorted = false;
  if (rc != GX_OK) return rc;
  ex->lastKernelMs = sumMs;
  ex->runPos.assign(ex->sortRuns.size(), 0);
  ex->spillSkip = saveOff;
  ex->spillRemaining = saveLim;
  ex->spillSorted = true;
  if (getenv("GX_DEBUG"))
    fprintf(stderr, "[gx] spill sort: %zu runs of <=%lld rows, %.3f ms device\n",
            ex->sortRuns.size(), (long long)runRows, sumMs);
  return GX_OK;
}

// decide between the in-HBM sort and the spill path (env override or HBM
// budget); GX_OK with spillSorted unset means: use the in-HBM path
static int32_t maybeSpillSort(gx_exec* ex) {
  auto it = ex->bindings.find(ex->sourceNode);
  if (it == ex->bindings.end() || it->second.haveChunks ||
      it->second.tpchTable < 0)
    return GX_OK;  // bound chunks are host-resident already: in-HBM path
  int64_t total = it->second.tpchRows;
  const PNode& srcN = ex->plan.nodes[ex->sourceNode];
  int64_t rowBytes = 0;
  for (int t : srcN.colTypes)
    rowBytes += t == GX_TYPE_DECIMAL ? 40 : (t == GX_TYPE_STRING ? 9 : 8);
  int64_t runRows = 0;
  if (const char* e = getenv("GX_SORT_RUN_ROWS")) runRows = atoll(e);
  if (runRows <= 0) {
    if (!gpuAvailable()) return GX_OK;  // NO_GPU surfaces on the normal path
    if (ex->device >= 0) hipSetDevice(ex->device);
    size_t freeB = 0, totB = 0;
    if (hipMemGetInfo(&freeB, &totB) != hipSuccess) return GX_OK;
    // in-HBM sort needs table + gathered copy + idx/key scratch (~24 B/row)
    double need = (double)total * (2.0 * rowBytes + 24.0);
    if (need < 0.6 * (double)freeB) return GX_OK;
    runRows = (int64_t)(0.25 * (double)freeB / (2.0 * rowBytes + 24.0));
    if (runRows < 1024) runRows = 1024;
  }
  if (total <= runRows) return GX_OK;
  return runDeviceSortSpill(ex, runRows);
}

// k-way merge emission over the host-resident sorted runs
// (multi_way_merge.go): composed u64 keys compare lexicographically
static int32_t emitSpillChunk(gx_exec* ex, gx_chunk* out, int32_t* rows_out) {
  const PNode& srcN = ex->plan.nodes[ex->sourceNode];
  int ncols = (int)srcN.colTypes.size();
  if (out->n_cols != ncols) {
    ex->err = "output chunk column count mismatch";
    return GX_ERR_INVALID;
  }
  int nk = (int)ex->devSortKeys.size();
  size_t R = ex->sortRuns.size();
  for (int c = 0; c < ncols; c++) {
    gx_col* g = &out->cols[c];
    int es = srcN.colTypes[c] == GX_TYPE_DECIMAL ? 40
             : (srcN.colTypes[c] == GX_TYPE_STRING ? 1 : 8);
    if (g->data_cap < 1024 * es ||
        (srcN.colTypes[c] == GX_TYPE_STRING && g->offsets_cap < 1025)) {
      ex->err = "output buffer too small";
      return GX_ERR_INVALID;
    }
    if (g->offsets) g->offsets[0] = 0;
  }
  int n = 0;
  while (n < 1024 && ex->spillRemaining != 0) {
    int best = -1;
    for (size_t r = 0; r < R; r++) {
      int64_t pos = ex->runPos[r];
      if (pos >= ex->sortRuns[r].n) continue;
      if (best < 0) {
        best = (int)r;
        continue;
      }
      const SortRun& a = ex->sortRuns[r];
      const SortRun& bs = ex->sortRuns[best];
      int64_t bpos = ex->runPos[best];
      for (int j = 0; j < nk; j++) {
        uint64_t ka = a.keys[j][pos], kb = bs.keys[j][bpos];
        if (ka < kb) { best = (int)r; break; }
        if (ka > kb) break;
      }
    }
    if (best < 0) break;
    int64_t pos = ex->runPos[best]++;
    if (ex->spillSkip > 0) {
      ex->spillSkip--;
      continue;
    }
    const SortRun& run = ex->sortRuns[best];
    for (int c = 0; c < ncols; c++) {
      gx_col* g = &out->cols[c];
      if (srcN.colTypes[c] == GX_TYPE_STRING) {
        ((uint8_t*)g->data)[n] = run.colData[c][pos];
        g->offsets[n + 1] = n + 1;
      } else {
        int es = srcN.colTypes[c] == GX_TYPE_DECIMAL ? 40 : 8;
        std::memcpy((uint8_t*)g->data + (size_t)n * es,
                    run.colData[c].data() + (size_t)pos * es, es);
      }
    }
    n++;
    if (ex->spillRemaining > 0) ex->spillRemaining--;
  }
  for (int c = 0; c < ncols; c++) {
    gx_col* g = &out->cols[c];
    if (g->null_bitmap) std::memset(g->null_bitmap, 0xFF, (n + 7) / 8);
    g->length = n;
  }
  out->n_rows = n;
  *rows_out = n;
  return GX_OK;
}

// emit the next <=1024 rows of the device-resident table in ex->desc.table
// (bare/sorted sources and joined-row output)
static int32_t emitTableChunk(gx_exec* ex, gx_chunk* out, int32_t* rows_out) {
  gxp::DevTable& tab = ex->desc.table;
  int64_t remaining = tab.nRows - ex->srcPos;
  int n = (int)std::min<int64_t>(remaining, 1024);
  if (n <= 0) {
    *rows_out = 0;
    return GX_OK;
  }
  if (out->n_cols != tab.nCols) {
    ex->err = "output chunk column count mismatch";
    return GX_ERR_INVALID;
  }
  for (int c = 0; c < tab.nCols; c++) {
    gxp::DevCol& col = tab.cols[c];
    gx_col* g = &out->cols[c];
    if (col.type == GX_TYPE_STRING) {
      std::vector<int64_t> offs(n + 1);
      HIP_OK(ex, hipMemcpy(offs.data(), col.offsets + ex->srcPos, (n + 1) * 8,
                           hipMemcpyDeviceToHost));
      int64_t base = offs[0];
      int64_t bytes = offs[n] - base;
      if (g->offsets_cap < n + 1 || g->data_cap < bytes) {
        ex->err = "output buffer too small";
        return GX_ERR_INVALID;
      }
      for (int i = 0; i <= n; i++) g->offsets[i] = offs[i] - base;
      HIP_OK(ex, hipMemcpy(g->data, (uint8_t*)col.data + base, bytes,
                           hipMemcpyDeviceToHost));
    } else {
      int64_t bytes = (int64_t)n * col.elemSize;
      if (g->data_cap < bytes) {
        ex->err = "output buffer too small";
        return GX_ERR_INVALID;
      }
      HIP_OK(ex, hipMemcpy(g->data, (uint8_t*)col.data + ex->srcPos * col.elemSize,
                           bytes, hipMemcpyDeviceToHost));
    }
    if (g->null_bitmap) {
      if (col.hasNulls && col.nullBitmap) {
        // srcPos advances in 1024-row steps AFTER the first chunk, but the
        // FIRST emission may start at a sort offset that is not a multiple
        // of 8 (runDeviceSort sets srcPos = devSortOffset): repack the
        // bitmap with the bit offset so NULL flags land on the right rows
        int bit = (int)(ex->srcPos & 7);
        if (bit == 0) {
          HIP_OK(ex, hipMemcpy(g->null_bitmap, col.nullBitmap + ex->srcPos / 8,
                               (n + 7) / 8, hipMemcpyDeviceToHost));
        } else {
          int nb = (n + bit + 7) / 8;  // source bytes covering [srcPos, srcPos+n)
          std::vector<uint8_t> tmp(nb + 1, 0);
          HIP_OK(ex, hipMemcpy(tmp.data(), col.nullBitmap + ex->srcPos / 8, nb,
                               hipMemcpyDeviceToHost));
          int outBytes = (n + 7) / 8;
          for (int i = 0; i < outBytes; i++)
            g->null_bitmap[i] =
                (uint8_t)((tmp[i] >> bit) | (tmp[i + 1] << (8 - bit)));
        }
      } else {
        std::memset(g->null_bitmap, 0xFF, (n + 7) / 8);
      }
    }
    g->length = n;
  }
  out->n_rows = n;
  ex->srcPos += n;
  *rows_out = n;
  return GX_OK;
}

// LimitExec (executor/limit.go): a keyless TOPN is a plain LIMIT/OFFSET —
// child row order preserved, offset rows skipped, limit rows kept
static void applyBareLimit(gx_exec* ex) {
  if (!ex->devSortKeys.empty() || ex->devSorted) return;
  if (ex->devSortLimit < 0 && ex->devSortOffset <= 0) return;
  int64_t n = ex->desc.table.nRows;
  ex->srcPos = ex->sliceStart = std::min<int64_t>(ex->devSortOffset, n);
  if (ex->devSortLimit >= 0)
    ex->desc.table.nRows = std::min<int64_t>(n, ex->srcPos + ex->devSortLimit);
  ex->devSorted = true;  // applied once
}

static int32_t emitSourceChunk(gx_exec* ex, gx_chunk* out, int32_t* rows_out) {
  // out-of-core sort decision comes BEFORE full materialization (spill runs
  // materialize row ranges themselves)
  if (!ex->devSortKeys.empty() && !ex->devSorted && !ex->spillSorted) {
    int32_t rc = maybeSpillSort(ex);
    if (rc) return rc;
  }
  if (ex->spillSorted) return emitSpillChunk(ex, out, rows_out);
  int32_t rc = materializeDevice(ex);
  if (rc) return rc;
  if (!ex->devSortKeys.empty() && !ex->devSorted) {
    rc = runDeviceSort(ex);
    if (rc) return rc;
  }
  applyBareLimit(ex);
  return emitTableChunk(ex, out, rows_out);
}

// ---------------- C ABI ----------------

// text form of one VM program (gx_debug_vm_program)
template <class Desc>
static void dumpVmProgram(std::string& s, const char* site, const Desc& d,
                          int nLoadIns, int nRegs, const gxp::FetchDesc* fetch,
                          int nFetch, int nLikePats) {
  // only the fused descriptor stores its register count
  if (nRegs < 0)
    for (int i = 0; i < d.nIns; i++) nRegs = std::max(nRegs, d.ins[i].dst + 1);
  char buf[256];
  snprintf(buf, sizeof buf, "site %s nIns=%d nLoadIns=%d nVmRegs=%d wide=%d\n",
           site, d.nIns, nLoadIns, nRegs, d.wide);
  s += buf;
  for (int i = 0; i < d.nIns; i++) {
    const gxp::VmIns& in = d.ins[i];
    snprintf(buf, sizeof buf,
             "ins[%d] op=%d dst=%d a=%d b=%d c=%d p10=%lld magic=%llu\n", i,
             in.op, in.dst, in.a, in.b, in.c, (long long)d.insP10[i],
             (unsigned long long)d.insMagic[i]);
    s += buf;
  }
  for (int i = 0; i < d.nConsts; i++) {
    snprintf(buf, sizeof buf, "const[%d] lo=%lld hi=%lld\n", i,
             (long long)d.constLo[i], (long long)d.constHi[i]);
    s += buf;
  }
  for (int i = 0; i < nFetch; i++) {
    snprintf(buf, sizeof buf, "fetch[%d] kind=%d col=%d\n", i, fetch[i].kind,
             fetch[i].col);
    s += buf;
  }
  snprintf(buf, sizeof buf, "likePats=%d\n", nLikePats);
  s += buf;
}

extern "C" {

gx_pb* gx_pb_new(void) { return new gx_pb(); }
void gx_pb_free(gx_pb* pb) { delete pb; }

static int32_t addExpr(gx_pb* pb, PExpr e) {
  pb->plan.exprs.push_back(std::move(e));
  return (int32_t)pb->plan.exprs.size() - 1;
}

int32_t gx_pb_colref(gx_pb* pb, int32_t col_idx, int32_t type, int32_t frac) {
  PExpr e;
  e.kind = EK_COLREF;
  e.colIdx = col_idx;
  e.retType = type;
  e.retFrac = frac;
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_const_i64(gx_pb* pb, int64_t v) {
  PExpr e;
  e.kind = EK_CONST;
  e.retType = GX_TYPE_I64;
  e.constI64 = v;
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_const_f64(gx_pb* pb, double v) {
  PExpr e;
  e.kind = EK_CONST;
  e.retType = GX_TYPE_F64;
  e.constF64 = v;
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_const_time(gx_pb* pb, uint64_t v) {
  PExpr e;
  e.kind = EK_CONST;
  e.retType = GX_TYPE_TIME;
  e.constTime = v;
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_const_dec(gx_pb* pb, const uint8_t dec40[40]) {
  PExpr e;
  e.kind = EK_CONST;
  e.retType = GX_TYPE_DECIMAL;
  std::memcpy(&e.constDec, dec40, 40);
  e.retFrac = e.constDec.resultFrac;
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_const_str(gx_pb* pb, const char* s, int32_t len) {
  PExpr e;
  e.kind = EK_CONST;
  e.retType = GX_TYPE_STRING;
  e.constStr.assign(s, len);
  return addExpr(pb, std::move(e));
}
int32_t gx_pb_call(gx_pb* pb, int32_t func, int32_t ret_type, int32_t ret_frac,
                   const int32_t* args, int32_t n_args) {
  PExpr e;
  e.kind = EK_CALL;
  e.func = func;
  e.retType = ret_type;
  e.retFrac = ret_frac < 0 ? 0 : ret_frac;
  for (int i = 0; i < n_args; i++) {
    if (args[i] < 0 || args[i] >= (int32_t)pb->plan.exprs.size())
      return GX_ERR_INVALID;
    e.args.push_back(args[i]);
  }
  return addExpr(pb, std::move(e));
}

static int32_t addNode(gx_pb* pb, PNode n) {
  pb->plan.nodes.push_back(std::move(n));
  return (int32_t)pb->plan.nodes.size() - 1;
}

int32_t gx_pb_source(gx_pb* pb, const int32_t* col_types, const int32_t* col_fracs,
                     int32_t n_cols) {
  PNode n;
  n.kind = PK_SOURCE;
  for (int i = 0; i < n_cols; i++) {
    n.colTypes.push_back(col_types[i]);
    n.colFracs.push_back(col_fracs ? col_fracs[i] : 0);
  }
  return addNode(pb, std::move(n));
}
int32_t gx_pb_selection(gx_pb* pb, int32_t child, const int32_t* conds,
                        int32_t n_conds) {
  PNode n;
  n.kind = PK_SELECTION;
  n.child = child;
  for (int i = 0; i < n_conds; i++) n.exprs.push_back(conds[i]);
  return addNode(pb, std::move(n));
}
int32_t gx_pb_projection(gx_pb* pb, int32_t child, const int32_t* exprs,
                         int32_t n_exprs) {
  PNode n;
  n.kind = PK_PROJECTION;
  n.child = child;
  for (int i = 0; i < n_exprs; i++) n.exprs.push_back(exprs[i]);
  return addNode(pb, std::move(n));
}
int32_t gx_pb_hashagg(gx_pb* pb, int32_t child, const int32_t* group_exprs,
                      int32_t n_group, const int32_t* agg_funcs,
                      const int32_t* agg_args, const int32_t* agg_fracs,
                      int32_t n_aggs, int32_t mode) {
  PNode n;
  n.kind = PK_HASHAGG;
  n.child = child;
  n.aggMode = mode;
  for (int i = 0; i < n_group; i++) n.exprs.push_back(group_exprs[i]);
  for (int i = 0; i < n_aggs; i++) {
    n.aggFuncs.push_back(agg_funcs[i]);
    n.aggArgs.push_back(agg_args[i]);
    n.aggFracs.push_back(agg_fracs ? agg_fracs[i] : 0);
  }
  return addNode(pb, std::move(n));
}
int32_t gx_pb_streamagg(gx_pb* pb, int32_t child, const int32_t* group_exprs,
                        int32_t n_group, const int32_t* agg_funcs,
                        const int32_t* agg_args, const int32_t* agg_fracs,
                        int32_t n_aggs) {
  PNode n;
  n.kind = PK_STREAMAGG;
  n.child = child;
  n.aggMode = GX_AGG_MODE_COMPLETE;
  for (int i = 0; i < n_group; i++) n.exprs.push_back(group_exprs[i]);
  for (int i = 0; i < n_aggs; i++) {
    n.aggFuncs.push_back(agg_funcs[i]);
    n.aggArgs.push_back(agg_args[i]);
    n.aggFracs.push_back(agg_fracs ? agg_fracs[i] : 0);
  }
  return addNode(pb, std::move(n));
}
int32_t gx_pb_topn(gx_pb* pb, int32_t child, const int32_t* key_exprs,
                   const uint8_t* key_desc, int32_t n_keys, int64_t limit,
                   int64_t offset) {
  PNode n;
  n.kind = PK_TOPN;
  n.child = child;
  for (int i = 0; i < n_keys; i++) {
    n.exprs.push_back(key_exprs[i]);
    n.keyDesc.push_back(key_desc ? key_desc[i] : 0);
  }
  n.limit = limit;
  n.offset = offset;
  return addNode(pb, std::move(n));
}
int32_t gx_pb_mergejoin(gx_pb* pb, int32_t build_child, int32_t probe_child,
                        const int32_t* build_keys, const int32_t* probe_keys,
                        int32_t n_keys, int32_t join_type) {
  PNode n;
  n.kind = PK_MERGEJOIN;
  n.child = build_child;
  n.child2 = probe_child;
  for (int i = 0; i < n_keys; i++) {
    n.buildKeys.push_back(build_keys[i]);
    n.probeKeys.push_back(probe_keys[i]);
  }
  n.joinType = join_type;
  return addNode(pb, std::move(n));
}
int32_t gx_pb_hashjoin(gx_pb* pb, int32_t build_child, int32_t probe_child,
                       const int32_t* build_keys, const int32_t* probe_keys,
                       int32_t n_keys, int32_t join_type) {
  PNode n;
  n.kind = PK_HASHJOIN;
  n.child = build_child;
  n.child2 = probe_child;
  n.joinType = join_type;
  for (int i = 0; i < n_keys; i++) {
    n.buildKeys.push_back(build_keys[i]);
    n.probeKeys.push_back(probe_keys[i]);
  }
  return addNode(pb, std::move(n));
}

// ---------------- plan routing ----------------
// gx_build peels the root of the plan into a PlanShape (classifyPlan), reads
// the route or ordered route list off it (routesFor) and compiles each route
// on a fresh executor over a pristine copy of the plan (compileRoute): the
// first success is the executor, and no attempt sees what another one did.

// [TopN] <- [HAVING] <- [HashAgg] <- ..., peeled. The only place these shape
// predicates live.
struct PlanShape {
  int topn = -1;    // the root, when it is a TopN / sort
  int body = -1;    // the node under it (the root itself when there is none)
  int having = -1;  // body, when it is a Selection over a non-FINAL HashAgg
  int agg = -1;     // that HashAgg, or body when it is a non-FINAL HashAgg
  // first node from body down that is no HashAgg, Projection or Selection
  int bottom = -1;
};

static PlanShape classifyPlan(const PPlan& plan, int root) {
  auto fusableAgg = [&](int n) {
    return plan.nodes[n].kind == PK_HASHAGG &&
           plan.nodes[n].aggMode != GX_AGG_MODE_FINAL;
  };
  PlanShape sh;
  sh.body = root;
  if (plan.nodes[root].kind == PK_TOPN) {
    sh.topn = root;
    sh.body = plan.nodes[root].child;
  }
  if (fusableAgg(sh.body)) {
    sh.agg = sh.body;
  } else if (plan.nodes[sh.body].kind == PK_SELECTION &&
             fusableAgg(plan.nodes[sh.body].child)) {
    sh.having = sh.body;
    sh.agg = plan.nodes[sh.body].child;
  }
  sh.bottom = sh.body;
  while (plan.nodes[sh.bottom].kind == PK_HASHAGG ||
         plan.nodes[sh.bottom].kind == PK_PROJECTION ||
         plan.nodes[sh.bottom].kind == PK_SELECTION)
    sh.bottom = plan.nodes[sh.bottom].child;
  return sh;
}

// the TopN's keys as columns of the aggregate's output, for the host sort
// over the decoded groups; false when one is anything else
static bool postSortKeysOf(const PPlan& plan, const PlanShape& sh,
                           std::vector<std::pair<int, bool>>* keys) {
  const PNode& topn = plan.nodes[sh.topn];
  const PNode& agg = plan.nodes[sh.agg];
  int aggWidth = (int)agg.exprs.size() + (int)agg.aggFuncs.size();
  keys->clear();
  for (size_t i = 0; i < topn.exprs.size(); i++) {
    const PExpr& ke = plan.exprs[topn.exprs[i]];
    if (ke.kind != EK_COLREF || ke.colIdx < 0 || ke.colIdx >= aggWidth)
      return false;
    keys->push_back({ke.colIdx, topn.keyDesc[i] != 0});
  }
  return true;
}

// device radix sort above a table of `types` columns (sortexec/sort.go:50,
// 546; stable LSD passes over composed u64 keys): the TopN's keys, limit and
// offset; `mustBe` is the complaint about a key that is no column of it
static bool composeDevSortKeys(gx_exec* ex, const PNode& topn,
                               const std::vector<int>& types,
                               const char* mustBe) {
  ex->devSortLimit = topn.limit;
  ex->devSortOffset = topn.offset;
  for (size_t i = 0; i < topn.exprs.size(); i++) {
    const PExpr& ke = ex->plan.exprs[topn.exprs[i]];
    if (ke.kind != EK_COLREF || ke.colIdx < 0 ||
        ke.colIdx >= (int)types.size()) {
      ex->err = mustBe;
      return false;
    }
    gxp::SortKeyCompose k{};
    k.col = ke.colIdx;
    k.desc = topn.keyDesc[i] != 0;
    int t = types[ke.colIdx];
    if (t == GX_TYPE_I64) k.kind = 0;
    else if (t == GX_TYPE_TIME) k.kind = 1;
    else if (t == GX_TYPE_STRING) k.kind = 2;  // dense char, or ranked at run
    else if (t == GX_TYPE_DECIMAL) k.kind = 3;
    else if (t == GX_TYPE_F64) k.kind = 5;
    else {
      ex->err = "unsupported sort key type this round";
      return false;
    }
    ex->devSortKeys.push_back(k);
  }
  return true;
}

// agg_stream_executor.go analog: semantics = grouped agg over a grouped
// stream, emitted in stream order. MI355X-first implementation: the sort
// below it is irrelevant to the aggregate VALUES, so run the fused hash
// aggregation over the sort's input and emit ordered by the sort keys --
// identical results, none of the sorted-input serialization.
static int32_t compileStreamAgg(gx_exec* ex, int node) {
  const PNode& sa = ex->plan.nodes[node];
  const PNode& sortn = ex->plan.nodes[sa.child];
  if (sortn.kind != PK_TOPN || sortn.limit >= 0) {
    ex->err = "device streamagg expects a full-sort child this round";
    return GX_ERR_INVALID;
  }
  // every sort key must be one of the group columns
  for (size_t i = 0; i < sortn.exprs.size(); i++) {
    const PExpr& ke = ex->plan.exprs[sortn.exprs[i]];
    int found = -1;
    for (size_t g = 0; g < sa.exprs.size(); g++) {
      const PExpr& ge = ex->plan.exprs[sa.exprs[g]];
      if (ke.kind == EK_COLREF && ge.kind == EK_COLREF &&
          ke.colIdx == ge.colIdx)
        found = (int)g;
    }
    if (found < 0) {
      ex->err = "streamagg sort keys must be group columns";
      return GX_ERR_INVALID;
    }
    ex->postSortKeys.push_back({found, sortn.keyDesc[i] != 0});
  }
  ex->postSort = true;
  PNode agg;
  agg.kind = PK_HASHAGG;
  agg.child = sortn.child;
  agg.aggMode = sa.aggMode;
  agg.exprs = sa.exprs;
  agg.aggFuncs = sa.aggFuncs;
  agg.aggArgs = sa.aggArgs;
  agg.aggFracs = sa.aggFracs;
  ex->plan.nodes.push_back(agg);  // invalidates sa and sortn
  return compileFused(ex, (int)ex->plan.nodes.size() - 1);
}

struct RouteList {
  ExecKind kinds[3];
  int n;
  const char* failed;  // the error when the last compiler left none
};

// The routing table: which compilers may take the shape, in order.
static RouteList routesFor(const PPlan& plan, const PlanShape& sh) {
  using K = ExecKind;
  static const char kPlanFailed[] = "plan compilation failed";
  static const char kJoinFailed[] = "join plan compilation failed";
  auto kindOf = [&](int n) { return plan.nodes[n].kind; };
  const bool sorted = sh.topn >= 0;
  const PNode& body = plan.nodes[sh.body];
  if (sh.agg >= 0) {
    // [TopN] <- [HAVING] <- HashAgg: the HAVING filter and the sort run on
    // the host over the (small) decoded group rows (the reference sorts the
    // agg output the same way -- Q1's final Sort, sortexec/sort.go)
    if (!sorted)
      return {{kindOf(sh.bottom) == PK_HASHJOIN ? K::AGG_OVER_JOIN : K::FUSED},
              1, kPlanFailed};
    // over a Source the join compilers have nothing to take
    if (kindOf(sh.bottom) == PK_SOURCE) return {{K::FUSED}, 1, kPlanFailed};
    std::vector<std::pair<int, bool>> keys;
    if (!postSortKeysOf(plan, sh, &keys))
      return {{K::JOIN_AGG}, 1, kPlanFailed};
    // fused aggregation; else the Q3-class join-aggregate pipeline; else
    // general aggregation over materialized joined rows
    return {{K::FUSED, K::JOIN_AGG, K::AGG_OVER_JOIN}, 3, kPlanFailed};
  }
  switch (body.kind) {
    case PK_SOURCE:  // bound table, sorted on device under a TopN
      return {{K::BARE_SOURCE}, 1, kPlanFailed};
    case PK_HASHJOIN:
      return {{K::HASH_JOIN}, 1, kJoinFailed};
    case PK_SELECTION:
      // post-join conditions, or the standalone Selection (SelectionExec);
      // under a TopN the materialized table feeds the device sort
      if (kindOf(body.child) == PK_HASHJOIN)
        return {{K::HASH_JOIN}, 1, kJoinFailed};
      if (sorted && kindOf(body.child) == PK_SOURCE)
        return {{K::SELECT}, 1, kJoinFailed};
      if (!sorted && kindOf(skipFullSort(plan, body.child)) == PK_SOURCE)
        return {{K::SELECT}, 1, kPlanFailed};
      break;
    case PK_HASHAGG:  // FINAL: the fusable ones are sh.agg
      if (!sorted) return {{K::FINAL_HOST}, 1, kPlanFailed};
      break;
    case PK_STREAMAGG:
      if (!sorted) return {{K::FUSED}, 1, kPlanFailed};
      break;
    case PK_PROJECTION:  // standalone Projection (ProjectionExec)
      if (!sorted) return {{K::PROJECT}, 1, kPlanFailed};
      break;
    default:
      break;
  }
  if (sorted) return {{K::JOIN_AGG}, 1, kJoinFailed};
  return {{K::NONE}, 1,
          "unsupported root plan node for the device engine this round"};
}

// Compiles ex's plan as route `k`; false with ex->err set when the route
// refuses it (empty = the route list's text applies). *stop: a plan error
// that no later route may paper over.
static bool compileRoute(gx_exec* ex, const PlanShape& sh, ExecKind k,
                         bool* stop) {
  PPlan& plan = ex->plan;
  *stop = true;
  if (!composedOnlyAtRootProjection(ex)) return false;
  if (sh.having >= 0 &&
      !compileHaving(ex, plan.nodes[sh.having].exprs, plan.nodes[sh.agg]))
    return false;
  *stop = false;
  // compilers append nodes to the plan: index it anew after one ran
  const bool sorted = sh.topn >= 0;
  switch (k) {
    case ExecKind::FUSED:
    case ExecKind::AGG_OVER_JOIN:
      if (plan.nodes[sh.body].kind == PK_STREAMAGG)
        return compileStreamAgg(ex, sh.body) == GX_OK;
      if (sorted) {
        if (!postSortKeysOf(plan, sh, &ex->postSortKeys)) {
          ex->err = "sort keys must be aggregate output columns";
          return false;
        }
        ex->postSort = true;
        ex->postLimit = plan.nodes[sh.topn].limit;  // -1 = full sort
        ex->postOffset = plan.nodes[sh.topn].offset;
      }
      return (k == ExecKind::FUSED ? compileFused(ex, sh.agg)
                                   : compileAggOverJoin(ex, sh.agg)) == GX_OK;
    case ExecKind::JOIN_AGG: {
      bool ok = compileJoinAgg(ex, ex->root) == GX_OK;
      *stop = ex->jaLikeRejected;
      return ok;
    }
    case ExecKind::FINAL_HOST: {
      const PNode& agg = plan.nodes[sh.body];
      if (plan.nodes[agg.child].kind != PK_SOURCE) {
        ex->err = "FINAL agg child must be a bound source";
        return false;
      }
      for (int f : agg.aggFuncs)
        if (f >= GX_AGG_COUNT_DISTINCT) {
          ex->err = "DISTINCT aggregates support COMPLETE mode only";
          return false;
        }
      ex->sourceNode = agg.child;
      return true;
    }
    case ExecKind::BARE_SOURCE: {
      const PNode& src = plan.nodes[sh.body];
      ex->sourceNode = sh.body;
      setTableMeta(&ex->desc.table, src.colTypes, src.colFracs);
      return !sorted ||
             composeDevSortKeys(ex, plan.nodes[sh.topn], src.colTypes,
                                "sort keys must be source columns");
    }
    case ExecKind::HASH_JOIN:
      if (compileHashJoinTree(ex, sh.body) != GX_OK) return false;
      return !sorted ||
             composeDevSortKeys(ex, plan.nodes[sh.topn],
                                ex->joinStages.back().types,
                                "sort keys must be join output columns");
    case ExecKind::SELECT:
      if (compileSelect(ex, sh.body) != GX_OK) return false;
      return !sorted ||
             composeDevSortKeys(ex, plan.nodes[sh.topn], ex->selStage.types,
                                "sort keys must be join output columns");
    case ExecKind::PROJECT:
      return compileProject(ex, sh.body) == GX_OK;
    case ExecKind::NONE:  // no route: only the checks every plan gets
      break;
  }
  return false;
}

gx_exec* gx_build(gx_pb* pb, int32_t root, int32_t device) {
  if (!pb || root < 0 || root >= (int32_t)pb->plan.nodes.size()) return nullptr;
  const PlanShape sh = classifyPlan(pb->plan, root);
  const RouteList routes = routesFor(pb->plan, sh);
  gx_exec* ex = nullptr;
  bool stop = false;
  for (int i = 0; i < routes.n && !stop; i++) {
    delete ex;  // a refused attempt: nothing of it reaches the next one
    ex = new gx_exec();
    ex->plan = pb->plan;
    ex->root = root;
    ex->device = device;
    if (compileRoute(ex, sh, routes.kinds[i], &stop)) {
      ex->kind = routes.kinds[i];
      return ex;
    }
  }
  if (ex->err.empty()) ex->err = routes.failed;
  return ex;
}

int32_t gx_bind_chunks(gx_exec* ex, int32_t source_node, const gx_chunk* chunks,
                       int32_t n_chunks) {
  if (!ex || source_node < 0 || source_node >= (int32_t)ex->plan.nodes.size())
    return GX_ERR_INVALID;
  const PNode& node = ex->plan.nodes[source_node];
  if (node.kind != PK_SOURCE) return GX_ERR_INVALID;
  Binding b;
  b.haveChunks = true;
  for (int i = 0; i < n_chunks; i++) {
    std::vector<HostCol> cols;
    if (chunks[i].n_cols != (int32_t)node.colTypes.size()) return GX_ERR_INVALID;
    for (int j = 0; j < chunks[i].n_cols; j++) {
      const gx_col& g = chunks[i].cols[j];
      HostCol hc;
      hc.type = node.colTypes[j];
      hc.frac = node.colFracs[j];
      hc.length = g.length;
      int nb = (g.length + 7) / 8;
      if (g.null_bitmap) hc.nullBitmap.assign(g.null_bitmap, g.null_bitmap + nb);
      else hc.nullBitmap.assign(nb, 0xFF);
      if (hc.type == GX_TYPE_STRING) {
        hc.offsets.assign(g.offsets, g.offsets + g.length + 1);
        hc.data.assign((uint8_t*)g.data, (uint8_t*)g.data + hc.offsets.back());
      } else {
        int es = hc.type == GX_TYPE_DECIMAL ? 40 : 8;
        hc.data.assign((uint8_t*)g.data, (uint8_t*)g.data + (size_t)g.length * es);
      }
      cols.push_back(std::move(hc));
    }
    b.chunks.push_back(std::move(cols));
  }
  ex->bindings[source_node] = std::move(b);
  return GX_OK;
}

int32_t gx_bind_tpch_sharded(gx_exec* ex, int32_t source_node, int32_t table,
                             int64_t n_rows, uint64_t seed, int64_t row_offset,
                             int64_t total_rows) {
  if (!ex || source_node < 0 || source_node >= (int32_t)ex->plan.nodes.size())
    return GX_ERR_INVALID;
  if (ex->plan.nodes[source_node].kind != PK_SOURCE) return GX_ERR_INVALID;
  Binding b;
  b.tpchTable = table;
  b.tpchRows = n_rows;
  b.tpchSeed = seed;
  b.tpchRowOffset = row_offset;
  b.tpchTotalRows = total_rows;
  ex->bindings[source_node] = std::move(b);
  return GX_OK;
}

int32_t gx_bind_tpch(gx_exec* ex, int32_t source_node, int32_t table,
                     int64_t n_rows, uint64_t seed, int64_t row_offset) {
  return gx_bind_tpch_sharded(ex, source_node, table, n_rows, seed, row_offset,
                              n_rows);
}

int32_t gx_open(gx_exec* ex) {
  if (!ex) return GX_ERR_INVALID;
  if (!ex->err.empty()) return GX_ERR_INVALID;
  if (ex->kind == ExecKind::NONE) {
    ex->err = "plan not executable";
    return GX_ERR_INVALID;
  }
  ex->ranQuery = false;
  ex->emitPos = 0;
  ex->srcPos = 0;
  ex->resultRows.clear();
  // join/select/project re-runs rebuild desc.table from scratch (beginRun
  // frees the previous run's buffers), so a sort above them must re-run too
  if (ex->kind == ExecKind::HASH_JOIN || ex->kind == ExecKind::SELECT ||
      ex->kind == ExecKind::PROJECT)
    ex->devSorted = false;
  // a bare source keeps its sorted (or limited) table, cut to offset + limit:
  // emission restarts at the slice's first row, the sort does not rerun
  if (ex->devSorted) ex->srcPos = ex->sliceStart;
  if (ex->spillSorted) {  // re-open: replay the merged runs from the top
    ex->runPos.assign(ex->sortRuns.size(), 0);
    ex->spillSkip = ex->devSortOffset;
    ex->spillRemaining = ex->devSortLimit;
  }
  ex->opened = true;
  return GX_OK;
}

// the query itself, once per open
static int32_t runQuery(gx_exec* ex) {
  switch (ex->kind) {
    case ExecKind::FUSED: return runFused(ex);
    case ExecKind::AGG_OVER_JOIN: {
      // materialize the joined rows, finish the fused bind over that table,
      // then aggregate (materializeDevice no-ops: runHashJoin set
      // deviceReady)
      int32_t rc = runHashJoin(ex);
      if (rc == GX_OK) rc = finalizeFusedBind(ex);
      if (rc == GX_OK) rc = runFused(ex);
      return rc;
    }
    case ExecKind::FINAL_HOST: return runFinalHost(ex);
    case ExecKind::JOIN_AGG: return runJoinAgg(ex);
    case ExecKind::HASH_JOIN: return runHashJoin(ex);
    case ExecKind::SELECT: return runSelect(ex);
    case ExecKind::PROJECT: return runProject(ex);
    case ExecKind::BARE_SOURCE:  // materializes as it emits
    case ExecKind::NONE: break;
  }
  return GX_OK;
}

int32_t gx_next(gx_exec* ex, gx_chunk* out, int32_t* rows_out) {
  if (!ex || !ex->opened) return GX_ERR_INVALID;
  if (ex->kind == ExecKind::BARE_SOURCE)
    return emitSourceChunk(ex, out, rows_out);
  auto fail = [&](int32_t rc) {
    *rows_out = 0;
    return rc;
  };
  if (!ex->ranQuery) {
    int32_t rc = runQuery(ex);
    if (rc) return fail(rc);
    ex->ranQuery = true;
  }
  if (ex->kind != ExecKind::HASH_JOIN && ex->kind != ExecKind::SELECT &&
      ex->kind != ExecKind::PROJECT)
    return gxp::emitRows(ex->resultRows, &ex->emitPos, out, rows_out, &ex->err);
  // a device table: sort it if keys are pending, cut it to the limit, emit;
  // only a HASH_JOIN spills (runHashJoin), one partition's output at a time
  const bool spill = ex->kind == ExecKind::HASH_JOIN && ex->joinSpill;
  if (!ex->devSortKeys.empty() && !ex->devSorted) {
    if (spill) {
      ex->err = "ORDER BY over an out-of-core join unsupported this round";
      return fail(GX_ERR_INVALID);
    }
    int32_t rc = runDeviceSort(ex);
    if (rc) return fail(rc);
  }
  if (spill && ex->devSortKeys.empty() && !ex->devSorted &&
      (ex->devSortLimit >= 0 || ex->devSortOffset > 0)) {
    ex->err = "LIMIT over an out-of-core join unsupported this round";
    return fail(GX_ERR_INVALID);
  }
  applyBareLimit(ex);
  int32_t rc = emitTableChunk(ex, out, rows_out);
  // out-of-core: stream the next partitions' outputs
  while (spill && rc == GX_OK && *rows_out == 0 &&
         ex->joinSpillCur < (int)ex->spillB.size()) {
    rc = joinSpillAdvance(ex);
    if (rc || ex->joinSpillCur >= (int)ex->spillB.size()) break;
    rc = emitTableChunk(ex, out, rows_out);
  }
  return rc;
}

int32_t gx_close(gx_exec* ex) {
  if (!ex) return GX_ERR_INVALID;
  ex->opened = false;
  return GX_OK;
}

void gx_exec_free(gx_exec* ex) { delete ex; }

const char* gx_last_error(gx_exec* ex) {
  if (!ex) return "null exec";
  return ex->err.c_str();
}

// debug: the hipRTC source the engine would generate for this plan
// (primarily for offline syntax checking; not part of the stable ABI)
const char* gx_debug_jit_source(gx_exec* ex) {
  static std::string s;
  if (!ex) return "";
  s = gxjit::generateSource(
      ex->desc, !ex->ldsNoRepl && !ex->desc.noLds && !getenv("GX_NO_LDS_REPL"));
  return s.c_str();
}

// debug: a text dump of the VM program the plan compiled to, at whichever of
// the three sites took it (works after gx_build without a GPU; pinned by
// tests/test_vm_programs.py; not part of the stable ABI)
const char* gx_debug_vm_program(gx_exec* ex) {
  static std::string s;
  s.clear();
  if (!ex) return "";
  if (ex->kind == ExecKind::JOIN_AGG) {
    int nLoads = 0;  // the probe kernel does not store it: leading loads
    while (nLoads < ex->ja.nIns && (ex->ja.ins[nLoads].op == gxp::VM_LOAD_DEC ||
                                    ex->ja.ins[nLoads].op == gxp::VM_LOAD_I64))
      nLoads++;
    dumpVmProgram(s, "probe", ex->ja, nLoads, -1, ex->ja.fetch, ex->ja.nFetch, 0);
  } else if (ex->kind == ExecKind::PROJECT) {
    dumpVmProgram(s, "projection", ex->pd, 0, -1, nullptr, 0, ex->pd.nLikePats);
    // composed string programs: a section of their own, only when present
    for (int ci = 0; ci < ex->pd.nCat; ci++) {
      const gxp::StrCatProg& cp = ex->pd.cat[ci];
      char buf[256];
      snprintf(buf, sizeof buf, "strcat[%d] nPieces=%d ws=%d sepOff=%d sepLen=%d\n",
               ci, cp.nPieces, cp.ws, cp.sepOff, cp.sepLen);
      s += buf;
      for (int p = 0; p < cp.nPieces; p++) {
        const gxp::StrPiece& pc = cp.piece[p];
        snprintf(buf, sizeof buf,
                 "piece[%d] kind=%d case=%d nWin=%d col=%d slot=%d constOff=%d "
                 "constLen=%d\n",
                 p, pc.kind, pc.caseOp, pc.nWin, pc.col, pc.slot, pc.constOff,
                 pc.constLen);
        s += buf;
        for (int w = 0; w < pc.nWin; w++) {
          snprintf(buf, sizeof buf, "win[%d] pos=%d len=%d\n", w, pc.winPos[w],
                   pc.winLen[w]);
          s += buf;
        }
      }
    }
    if (ex->pd.nCat > 0) s += "strcatPool=" + std::to_string(ex->pd.catPoolLen) + "\n";
  } else if (ex->usesFusedDesc()) {
    dumpVmProgram(s, "fused", ex->desc, ex->desc.nLoadIns, ex->desc.nVmRegs,
                  ex->desc.fetch, ex->desc.nFetch, ex->desc.nLikePats);
  } else {
    s = "site none\nerror: " + ex->err + "\n";
  }
  return s.c_str();
}

// debug: one composed string output over one host chunk, on the host, through
// gx_strcat.h's passes (length, prefix sum, tile-by-tile byte mapping) --
// the source the kernels run; no GPU needed
int32_t gx_debug_strcat_eval(gx_exec* ex, int32_t out_col, const gx_chunk* in,
                             gx_col* out) {
  if (!ex || !in || !out) return GX_ERR_INVALID;
  if (ex->kind != ExecKind::PROJECT || out_col < 0 || out_col >= (int)ex->projOutCat.size() ||
      ex->projOutCat[out_col] < 0) {
    ex->err = "gx_debug_strcat_eval: not a composed string output";
    return GX_ERR_INVALID;
  }
  const gxp::ProjDesc& pd = ex->pd;
  const gxp::StrCatProg& cp = pd.cat[ex->projOutCat[out_col]];
  const std::vector<int>& types = ex->projOverSelect
                                      ? ex->selStage.types
                                      : ex->plan.nodes[ex->projSrcNode].colTypes;
  if (in->n_cols != (int32_t)types.size() || in->n_rows < 0) {
    ex->err = "gx_debug_strcat_eval: chunk does not match the input schema";
    return GX_ERR_INVALID;
  }
  gxp::StrCatHostSrc src;
  src.poolp = pd.catPool;
  for (int p = 0; p < cp.nPieces; p++) {
    const gxp::StrPiece& pc = cp.piece[p];
    if (pc.kind == gxp::SPK_CONST) continue;
    if (pc.col < 0) {
      ex->err = "gx_debug_strcat_eval: a VM-computed CAST_STR argument needs "
                "the device";
      return GX_ERR_INVALID;
    }
    const gx_col& g = in->cols[pc.col];
    src.nullBitmap[p] = g.null_bitmap;
    if (pc.kind == gxp::SPK_I64) {
      src.i64[p] = (const int64_t*)g.data;
    } else {
      src.data[p] = (const uint8_t*)g.data;
      src.offsets[p] = g.offsets;
    }
  }
  int64_t n = in->n_rows;
  std::vector<int64_t> lens(n), off(n + 1, 0);
  std::vector<uint8_t> notNull(n);
  if (!gxp::strCatHostLens(cp, src, n, lens.data(), notNull.data())) {
    ex->err = "a CONCAT / CONCAT_WS output row exceeds 2 GiB";
    return GX_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; i++) off[i + 1] = off[i] + lens[i];
  if (out->offsets_cap < n + 1 || out->data_cap < off[n]) {
    ex->err = "output buffer too small";
    return GX_ERR_INVALID;
  }
  gxp::strCatHostEmit(cp, src, n, off.data(), (uint8_t*)out->data);
  for (int64_t i = 0; i <= n; i++) out->offsets[i] = off[i];
  if (out->null_bitmap) {
    std::memset(out->null_bitmap, 0, (n + 7) / 8);
    for (int64_t i = 0; i < n; i++)
      if (notNull[i]) out->null_bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
  }
  out->length = (int32_t)n;
  return GX_OK;
}

// debug: decimal columns currently served from an int64 units column (fused
// table + join-agg probe); 0 when every decimal still reads the 40 B form
int32_t gx_debug_dec_units_cols(gx_exec* ex) {
  return ex ? ex->decUnitsFused + ex->decUnitsJa : 0;
}

// debug: bytes per row of source column `col`'s units column in the fused
// table or the join-agg probe table; 0 when it is not served from units
int32_t gx_debug_dec_units_width(gx_exec* ex, int32_t col) {
  if (!ex || col < 0 || col >= gxp::kMaxCols) return 0;
  const gxp::DevCol& c =
      (ex->kind == ExecKind::JOIN_AGG ? ex->ja.probe : ex->desc.table)
          .cols[col];
  return c.units ? c.unitsWidth : 0;
}

// debug: rows per lane per load of the kernel that ran the last fused pass
// (recorded when its source was generated; 1 for the interpreted kernels,
// 0 before any pass)
int32_t gx_debug_rows_per_lane(gx_exec* ex) {
  return ex ? ex->lastRowsPerLane : 0;
}

// debug: accumulation tier of the last fused pass -- 0 lane-replicated LDS
// accumulators, 1 single 64-slot LDS table, 2 global-direct; -1 before one
int32_t gx_debug_lds_tier(gx_exec* ex) { return ex ? ex->lastLdsTier : -1; }

// debug: 1 when the last fused decode read its groups from the compact result
// block, 0 when it took the full-table download
int32_t gx_debug_result_compact(gx_exec* ex) {
  return ex && ex->lastDecodeCompact ? 1 : 0;
}

// debug: group slots of the replicated LDS table for this plan (0 = none)
int32_t gx_debug_lds_repl_slots(gx_exec* ex) {
  return ex && ex->usesFusedDesc() ? gxjit::replSlots(ex->desc) : 0;
}

double gx_last_kernel_ms(gx_exec* ex) { return ex ? ex->lastKernelMs : 0; }
int64_t gx_last_sel_count(gx_exec* ex) {
  return ex ? (int64_t)ex->lastSelCount : 0;
}

int32_t gx_engine_is_gpu(void) { return 1; }
const char* gx_engine_name(void) { return "gxexec-mi355x"; }

}  // extern "C"
