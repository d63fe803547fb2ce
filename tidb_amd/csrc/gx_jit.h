// runtime kernel specialization via hipRTC (see gx_jit.cpp)
#pragma once
#include <string>
#include "gx_common.h"

namespace gxjit {
struct JitProg;
// compile (process-cached) a specialized fused-agg kernel for this plan;
// nullptr (with *whyNot set) on any failure -- caller falls back to the
// interpreted kernel
// repl = the lane-replicated LDS layout (first accumulation tier): a small
// key table whose accumulators have R copies; a block that meets more keys
// than it holds raises kErrLdsSmall and the engine reruns with repl = false
const JitProg* compile(const gxp::FusedQueryDesc& d, bool repl,
                       std::string* whyNot);
// group slots of the replicated layout for this plan (0 = it has none)
int replSlots(const gxp::FusedQueryDesc& d);
// rows a lane of the generated kernel takes per load for this plan (1 = the
// one-row loop; GX_ROWS_PER_LANE picks 1, 2 or 4)
int rowsPerLane(const gxp::FusedQueryDesc& d);
// rows per lane the compiled program was generated with
int progRowsPerLane(const JitProg* prog);
int launch(const JitProg* prog, bool wide, const gxp::FusedQueryDesc* devDesc,
           int grid, void* stream);
std::string generateSource(const gxp::FusedQueryDesc& d, bool repl);
// join-aggregate probe kernel specialization
const JitProg* compileJa(const gxp::JoinAggDesc& d, std::string* whyNot);
int launchJa(const JitProg* prog, bool wide, const gxp::JoinAggDesc* devDesc,
             int grid, void* stream);
// join-aggregate build-phase kernels (count0/build0/count1/build1)
struct JaBuildProg;
const JaBuildProg* compileJaBuild(const gxp::JoinAggDesc& d,
                                  std::string* whyNot);
int launchJaBuild(const JaBuildProg* prog, int phase,
                  const gxp::JoinAggDesc* devDesc, int grid, void* stream);
}  // namespace gxjit
