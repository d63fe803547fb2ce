// tidb_amd/csrc/gx_result.h — host result stage: everything between "the
// group states are on the host" and "rows are in the caller's chunk".
//
// Pure functions over rows of OutRowVal: no HIP, no executor state. Inputs
// are explicit (rows, specs, an error string), so tools/result_stage_check.cpp
// drives every function under ASan+UBSan without a GPU. O(#groups) work.
#ifndef GXP_RESULT_H
#define GXP_RESULT_H

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gx_executor.h"
#include "gx_decimal.h"

namespace gxp {

// one result cell; `type` selects the member that holds the value
struct OutRowVal {
  bool isNull = false;
  int type = GX_TYPE_I64;
  int64_t i64 = 0;
  uint64_t u64 = 0;
  double f64 = 0;
  MyDecimal dec;
  std::string str;
};
using ResultRow = std::vector<OutRowVal>;

// host copy of one bound chunk column
struct HostCol {
  int type, frac;
  std::vector<uint8_t> data;
  std::vector<uint8_t> nullBitmap;
  std::vector<int64_t> offsets;
  int length = 0;
};

// int128 units at `scale` -> canonical MyDecimal (digit-exact value)
MyDecimal decFromUnits(__int128 u, int scale);

// ORDER: the SQL ordering of two cells of one type, for ORDER BY, HAVING
// leaves and the MIN/MAX merge. NULL first, TIME without its low 4 bits,
// strings under PAD SPACE.
int cmpOrder(const OutRowVal& a, const OutRowVal& b);
// IDENTITY: "the same stored value", for the DISTINCT fold's sets. NULL
// first, raw TIME bits, untrimmed strings.
int cmpIdentity(const OutRowVal& a, const OutRowVal& b);

// SUM / AVG finalize (func_sum.go:203-222, func_avg.go:84-109): NULL when
// cnt == 0; SUM[_DISTINCT] rounds half-up to `frac`; anything else is an
// average: sum / cnt with four more fraction digits (DivPrecisionIncrement),
// then the same round. False when the division fails; the caller owns the
// error text.
bool finalizeDecimalAgg(int func, const MyDecimal& sum, int64_t cnt, int frac,
                        OutRowVal* out);
void finalizeF64Agg(int func, double sum, int64_t cnt, OutRowVal* out);

// DISTINCT fold: rows are unique (keys..., args...) combinations; fold them
// to (keys..., one value per aggregate) in first-seen group order
struct DistinctSpec {
  int nKeys = -1;                         // -1 = not a DISTINCT query
  std::vector<int> funcs, fracs;          // per user aggregate
  std::vector<std::vector<int>> argSlot;  // per aggregate: its arg columns
};
int32_t foldDistinct(std::vector<ResultRow>* rows, const DistinctSpec& spec,
                     std::string* err);

// HAVING, compiled at build time: the conjuncts AND together, each one an OR
// of leaves in left-to-right order
struct HavingLeaf {
  int col = -1;
  int cmp = GX_F_EQ;        // already mirrored for <const cmp col>
  bool isNullTest = false;  // IS [NOT] NULL(col)
  bool wantNull = false;
  OutRowVal cst;
};
using HavingCond = std::vector<HavingLeaf>;
// VecEvalBool semantics: a NULL value rejects its leaf. *typeOk goes false
// when a leaf that is actually reached pairs a value and a constant the
// stage cannot compare; the row's verdict is then meaningless.
bool havingPass(const ResultRow& row, const std::vector<HavingCond>& conds,
                bool* typeOk);

// stable sort by (column, descending) keys, then OFFSET / LIMIT (-1 = all)
void sortAndSlice(std::vector<ResultRow>* rows,
                  const std::vector<std::pair<int, bool>>& keys,
                  int64_t offset, int64_t limit);

// marshal up to 1024 rows from *pos into the caller's chunk; advances *pos
int32_t emitRows(const std::vector<ResultRow>& rows, size_t* pos,
                 gx_chunk* out, int32_t* rowsOut, std::string* err);

// decode cell i of a bound chunk column; fills only the member(s) of the
// column's type (f64 for F64; u64 and i64 for I64/TIME)
OutRowVal readCell(const HostCol& hc, int i);

// FINAL-mode merge of canonical partial states (MergePartialResult
// semantics, aggfuncs.go:250-255) in first-seen group order
struct FinalSpec {
  size_t nGroup = 0;
  std::vector<int> funcs, fracs;
  std::vector<uint8_t> argIsF64;  // SUM/AVG over an f64 argument
};
int32_t mergeFinal(const std::vector<std::vector<HostCol>>& chunks,
                   const FinalSpec& spec, std::vector<ResultRow>* rows,
                   std::string* err);

}  // namespace gxp
#endif
