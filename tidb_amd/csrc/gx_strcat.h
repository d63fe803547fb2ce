// tidb_amd/csrc/gx_strcat.h — composed string outputs of the device
// Projection (CONCAT / CONCAT_WS / CAST(int AS CHAR)): the descriptor, the
// per-row piece table and the output-byte mapping, shared by the host plan
// compiler, the two kernels, the host evaluator (gx_debug_strcat_eval) and
// tools/strcat_check.cpp.
//
// A composed string is a list of at most kStrCatMaxPieces pieces. A piece is
// a windowed view of a string column (the SUBSTR/UPPER/LOWER/TRIM fold of
// the single-column path), a constant from the operator's pool, or the
// decimal text of an int64. Byte semantics throughout (builtinConcatSig,
// builtinConcatWSSig, builtinCastIntAsStringSig).
//
// Two passes, no per-piece temporaries in between:
//   length pass  strCatRow()        -> lens[row], notNull[row]
//   (exclusive sum of lens -> offsets)
//   emit pass    strCatRow() again into a per-tile table, then every aligned
//                word of the tile's output finds (row, piece, source byte)
//                for its bytes with strCatWord(): strCatFindRow() once, then
//                strCatByte() per byte.
// Sources are reached through an accessor type `Src` (device: DevCol loads;
// host: plain pointers):
//   bool    strNull(int piece, int64_t row)
//   void    strRange(int piece, int64_t row, int64_t* start, int64_t* len)
//   uint8_t strByte(int piece, int64_t idx)        // byte of the column data
//   bool    i64At(int piece, int64_t row, int64_t* v)  // false = NULL
//   uint8_t pool(int idx)                          // constant pool byte
#ifndef GX_STRCAT_H
#define GX_STRCAT_H

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define GX_SC_HD __host__ __device__
#else
#define GX_SC_HD
#endif

namespace gxp {

constexpr int kStrCatMaxPieces = 8;    // per output, after flattening
constexpr int kStrCatPoolBytes = 256;  // string constants per operator
constexpr int kStrCatTile = 256;       // rows per emit tile
constexpr int kStrCatMaxWin = 4;       // window steps per piece (kMaxStrWin)
// a composed row holds at most this many bytes (tile tables keep piece ends
// in 32 bits); a longer row raises the operator's error flag
constexpr int64_t kStrCatMaxRowBytes = 0x7FFFFFFF;

enum StrPieceKind : uint8_t { SPK_WINDOW = 0, SPK_CONST = 1, SPK_I64 = 2 };
enum StrCaseOp : uint8_t { SCO_NONE = 0, SCO_UPPER = 1, SCO_LOWER = 2 };

struct StrPiece {
  uint8_t kind = SPK_CONST;
  uint8_t caseOp = SCO_NONE;  // WINDOW: outermost ASCII case op
  uint8_t nWin = 0;           // WINDOW: window steps
  uint8_t pad = 0;
  int16_t col = -1;   // WINDOW: string column; I64: int64 column, or -1
  int16_t slot = -1;  // I64 with col < 0: hidden computed output of the VM
  uint16_t constOff = 0, constLen = 0;  // CONST: range of the pool
  // window steps as in StrProg (1-based pos, negative from the end, len -1 =
  // a TRIM step), saturated to 32 bits: a source row is shorter than 2 GiB
  int32_t winPos[kStrCatMaxWin] = {0, 0, 0, 0};
  int32_t winLen[kStrCatMaxWin] = {0, 0, 0, 0};
};

struct StrCatProg {
  StrPiece piece[kStrCatMaxPieces];
  uint8_t nPieces = 0;
  uint8_t ws = 0;  // CONCAT_WS: NULL pieces drop with their separator
  uint16_t sepOff = 0, sepLen = 0;  // CONCAT_WS separator in the pool
  uint16_t pad = 0;
};

// ---- window fold (builtinSubstring3ArgsSig / builtinTrim1ArgSig, byte
// semantics): SUBSTR windows compose, a both-ends space strip stays a window.
// (s, len) enters as the row's byte range and leaves as the view's.
template <class P, class ByteAt>
GX_SC_HD inline void strWindowFold(int nWin, const P* winPos, const P* winLen,
                                   int64_t* sIo, int64_t* lenIo,
                                   const ByteAt& byteAt) {
  int64_t s = *sIo, len = *lenIo;
  for (int w = 0; w < nWin; w++) {
    int64_t pos = winPos[w], L = winLen[w];
    if (L == -1) {  // TRIM
      while (len > 0 && byteAt(s) == ' ') { s++; len--; }
      while (len > 0 && byteAt(s + len - 1) == ' ') len--;
      continue;
    }
    // 1-based pos, negative from the end, out-of-range / len <= 0 -> empty
    int64_t start = pos < 0 ? len + pos + 1 : pos;
    if (start < 1 || start > len || L <= 0) {
      len = 0;
      break;
    }
    int64_t l2 = L < len - (start - 1) ? L : len - (start - 1);
    s += start - 1;
    len = l2;
  }
  *sIo = s;
  *lenIo = len;
}

// int64 window argument -> the 32-bit descriptor field
inline int32_t strWinSaturate(int64_t v) {
  if (v > 0x7FFFFFFFLL) return 0x7FFFFFFF;
  if (v < -0x7FFFFFFFLL) return -0x7FFFFFFF;
  return (int32_t)v;
}

// ---- decimal text of an int64 (builtinCastIntAsStringSig, signed): the
// magnitude is taken in uint64_t, so INT64_MIN needs no signed negation
GX_SC_HD inline uint64_t i64Magnitude(int64_t v) {
  uint64_t u = (uint64_t)v;
  return v < 0 ? (uint64_t)0 - u : u;
}

GX_SC_HD inline int u64Digits(uint64_t a) {
  int d = 1;
  uint64_t p = 10;
  while (a >= p) {
    d++;
    if (d == 20) break;  // 10^19 is the last power below 2^64
    p *= 10;
  }
  return d;
}

// bytes of the text, '-' included
GX_SC_HD inline int i64TextLen(int64_t v) {
  return u64Digits(i64Magnitude(v)) + (v < 0 ? 1 : 0);
}

// byte j of the text, textLen = i64TextLen(v), 0 <= j < textLen. Digits
// come off the right end by constant divisions (multiplies on the device).
GX_SC_HD inline uint8_t i64TextByte(int64_t v, int textLen, int j) {
  if (v < 0 && j == 0) return (uint8_t)'-';
  uint64_t a = i64Magnitude(v);
  int k = textLen - 1 - j;  // digit index from the right
  for (int i = 0; i < k; i++) a /= 10;
  return (uint8_t)('0' + a % 10);
}

GX_SC_HD inline uint8_t strApplyCase(uint8_t b, uint8_t caseOp) {
  if (caseOp == SCO_UPPER && b >= 'a' && b <= 'z') return (uint8_t)(b - 'a' + 'A');
  if (caseOp == SCO_LOWER && b >= 'A' && b <= 'Z') return (uint8_t)(b - 'A' + 'a');
  return b;
}

// ---- per-row piece table. For each piece p, in order, the sink receives
// put(p, start, end):
//   start  WINDOW: first byte of the view in the column data; CONST: pool
//          offset; I64: the value itself
//   end    bytes of the output row up to and including piece p's segment. A
//          segment is the piece's bytes, preceded under CONCAT_WS by the
//          separator when a non-NULL piece came before; a NULL piece has an
//          empty segment.
// then mask(m): bit p set = piece p is not NULL. Returns the row's byte
// length; *notNull = 0 for a NULL row (CONCAT with any NULL piece), whose
// length is 0 and whose table is never read. A row longer than
// kStrCatMaxRowBytes returns -1.
template <class Src, class Sink>
GX_SC_HD inline int64_t strCatRow(const StrCatProg& pg, const Src& src,
                                  int64_t row, Sink& sink, uint8_t* notNull) {
  int64_t total = 0;
  uint32_t m = 0;
  bool rowNull = false;
  for (int p = 0; p < pg.nPieces; p++) {
    const StrPiece& pc = pg.piece[p];
    int64_t s = 0, len = 0;
    bool nul = false;
    if (pc.kind == SPK_CONST) {
      s = pc.constOff;
      len = pc.constLen;
    } else if (pc.kind == SPK_I64) {
      int64_t v = 0;
      nul = !src.i64At(p, row, &v);
      if (!nul) {
        s = v;
        len = i64TextLen(v);
      }
    } else {
      nul = src.strNull(p, row);
      if (!nul) {
        src.strRange(p, row, &s, &len);
        strWindowFold(pc.nWin, pc.winPos, pc.winLen, &s, &len,
                      [&](int64_t i) { return src.strByte(p, i); });
      }
    }
    if (nul) {
      if (!pg.ws) rowNull = true;
      s = 0;
    } else {
      if (pg.ws && m != 0) total += pg.sepLen;
      m |= 1u << p;
      total += len;
    }
    sink.put(p, s, total);
  }
  sink.mask(m);
  *notNull = rowNull ? 0 : 1;
  if (rowNull) return 0;
  return total > kStrCatMaxRowBytes ? -1 : total;
}

// sink of the length pass: keeps nothing
struct StrCatNoSink {
  GX_SC_HD void put(int, int64_t, int64_t) {}
  GX_SC_HD void mask(uint32_t) {}
};

// ---- output byte -> row. off[0..T] are the tile's output offsets and
// off[0] <= g < off[T]; returns the row r with off[r] <= g < off[r+1]. Rows
// of length 0 (empty or NULL) have off[r] == off[r+1] and are never returned.
template <class Off>
GX_SC_HD inline int strCatFindRow(const Off& off, int T, int64_t g) {
  int lo = 0, hi = T;  // off[lo] <= g < off[hi]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- byte q of tile row r (0 <= q < row length). `tab` is the tile's piece
// table as strCatRow wrote it: start(p, r), end(p, r), mask(r).
template <class Src, class Tab>
GX_SC_HD inline uint8_t strCatByte(const StrCatProg& pg, const Src& src,
                                   const Tab& tab, int r, int64_t q) {
  int p = 0;
  int64_t segStart = 0;
  while (p < pg.nPieces - 1) {
    int64_t e = tab.end(p, r);
    if (q < e) break;
    segStart = e;
    p++;
  }
  int64_t j = q - segStart;
  int64_t len = tab.end(p, r) - segStart;  // the piece's own bytes
  if (pg.ws && (tab.mask(r) & ((1u << p) - 1u)) != 0) {
    if (j < pg.sepLen) return src.pool(pg.sepOff + (int)j);
    j -= pg.sepLen;
    len -= pg.sepLen;
  }
  const StrPiece& pc = pg.piece[p];
  if (pc.kind == SPK_CONST) return src.pool(pc.constOff + (int)j);
  if (pc.kind == SPK_I64)
    return i64TextByte(tab.start(p, r), (int)len, (int)j);
  return strApplyCase(src.strByte(p, tab.start(p, r) + j), pc.caseOp);
}

// ---- output bytes [lo, hi) of a tile, hi - lo <= 4, all inside the aligned
// word at w (w <= lo, hi <= w + 4): one row search, then a walk along the
// rows. Byte g lands at bits [8 (g - w), 8 (g - w) + 8) of the result, so a
// full word stores in one piece.
template <class Src, class Tab, class Off>
GX_SC_HD inline uint32_t strCatWord(const StrCatProg& pg, const Src& src,
                                    const Tab& tab, const Off& off, int T,
                                    int64_t w, int64_t lo, int64_t hi) {
  int r = strCatFindRow(off, T, lo);
  uint32_t word = 0;
  for (int64_t g = lo; g < hi; g++) {
    while (g >= off[r + 1]) r++;  // g < off[T]: stops at a row with bytes
    word |= (uint32_t)strCatByte(pg, src, tab, r, g - off[r])
            << (8 * (int)(g - w));
  }
  return word;
}

// ================= host drivers =================
// The evaluator and the stand-alone check run the kernels' passes through
// these: length pass, then (after the caller's prefix sum) the tile-by-tile
// byte mapping with T = kStrCatTile.

struct StrCatHostTab {
  int64_t startv[kStrCatMaxPieces][kStrCatTile];
  uint32_t endv[kStrCatMaxPieces][kStrCatTile];
  uint8_t maskv[kStrCatTile];
  int64_t start(int p, int r) const { return startv[p][r]; }
  int64_t end(int p, int r) const { return endv[p][r]; }
  uint32_t mask(int r) const { return maskv[r]; }
};

struct StrCatHostSink {
  StrCatHostTab* t;
  int r;
  void put(int p, int64_t s, int64_t e) {
    t->startv[p][r] = s;
    t->endv[p][r] = (uint32_t)e;
  }
  void mask(uint32_t m) { t->maskv[r] = (uint8_t)m; }
};

// length pass over rows [0, n): lens[n], notNull[n] (1 = NOT NULL). Returns
// false when a row exceeds kStrCatMaxRowBytes.
template <class Src>
inline bool strCatHostLens(const StrCatProg& pg, const Src& src, int64_t n,
                           int64_t* lens, uint8_t* notNull) {
  bool ok = true;
  for (int64_t row = 0; row < n; row++) {
    StrCatNoSink sink;
    uint8_t nn = 0;
    int64_t len = strCatRow(pg, src, row, sink, &nn);
    if (len < 0) {
      ok = false;
      len = 0;
      nn = 0;
    }
    lens[row] = len;
    notNull[row] = nn;
  }
  return ok;
}

// emit pass: off[n+1] is the exclusive sum of lens; out holds off[n] bytes
template <class Src>
inline void strCatHostEmit(const StrCatProg& pg, const Src& src, int64_t n,
                           const int64_t* off, uint8_t* out) {
  StrCatHostTab tab;
  for (int64_t r0 = 0; r0 < n; r0 += kStrCatTile) {
    int T = n - r0 < kStrCatTile ? (int)(n - r0) : kStrCatTile;
    for (int r = 0; r < T; r++) {
      StrCatHostSink sink{&tab, r};
      uint8_t nn = 0;
      (void)strCatRow(pg, src, r0 + r, sink, &nn);
    }
    const int64_t* toff = off + r0;
    // word by word, as the emit kernel's lanes do
    for (int64_t w = toff[0] & ~(int64_t)3; w < toff[T]; w += 4) {
      int64_t lo = w < toff[0] ? toff[0] : w;
      int64_t hi = w + 4 < toff[T] ? w + 4 : toff[T];
      uint32_t word = strCatWord(pg, src, tab, toff, T, w, lo, hi);
      for (int64_t g = lo; g < hi; g++)
        out[g] = (uint8_t)(word >> (8 * (int)(g - w)));
    }
  }
}

// plain-pointer accessor for the host drivers: one entry per piece
struct StrCatHostSrc {
  const uint8_t* data[kStrCatMaxPieces] = {};       // WINDOW: column bytes
  const int64_t* offsets[kStrCatMaxPieces] = {};    // WINDOW: n+1 offsets
  const uint8_t* nullBitmap[kStrCatMaxPieces] = {}; // LSB-first, 1 = NOT NULL;
                                                    // null = no NULLs
  const int64_t* i64[kStrCatMaxPieces] = {};        // I64: values
  const uint8_t* poolp = nullptr;
  bool isNull(int p, int64_t row) const {
    return nullBitmap[p] && ((nullBitmap[p][row >> 3] >> (row & 7)) & 1) == 0;
  }
  bool strNull(int p, int64_t row) const { return isNull(p, row); }
  void strRange(int p, int64_t row, int64_t* s, int64_t* len) const {
    *s = offsets[p][row];
    *len = offsets[p][row + 1] - *s;
  }
  uint8_t strByte(int p, int64_t idx) const { return data[p][idx]; }
  bool i64At(int p, int64_t row, int64_t* v) const {
    if (isNull(p, row)) return false;
    *v = i64[p][row];
    return true;
  }
  uint8_t pool(int i) const { return poolp[i]; }
};

}  // namespace gxp

#endif  // GX_STRCAT_H
