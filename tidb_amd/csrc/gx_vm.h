// gx_vm.h — the one device definition of the expression VM's opcodes.
// Included at the end of gx_device.h, so the interpreters in gx_kernels.hip
// and every hipRTC-generated kernel (gx_jit.cpp) compute from the same text.
//
// Layer 1: value functions on plain typename VT<WIDE>::T operands. The
// interpreters call them with runtime operands, generated code with literals.
// Layer 2: vmStep, one interpreter step for every opcode that is not a load.
// Loads (VM_LOAD_DEC, VM_LOAD_I64, VM_STRLEN, VM_LIKE) stay with each kernel:
// they reach column data through that kernel's own fetch plan.
#pragma once

namespace gxp {

template <bool WIDE>
__device__ inline __int128 vmToI128(typename VT<WIDE>::T v) {
  Int128 a = VT<WIDE>::toAcc(v);
  return ((__int128)a.hi << 64) | (__int128)a.lo;
}

// store a signed 128-bit result; a narrow VM whose result needs more than 64
// bits flags the wide retry and returns false
template <bool WIDE>
__device__ inline bool vmFromI128(__int128 q, typename VT<WIDE>::T* out,
                                  uint32_t* err) {
  if constexpr (WIDE) {
    *out = Int128{(uint64_t)q, (int64_t)(q >> 64)};
  } else {
    if (q != (__int128)(int64_t)q) {
      atomicOr(err, kErrRetryWide);
      return false;
    }
    *out = (int64_t)q;
  }
  return true;
}

// engine guarantees narrow-mode consts fit i64 (else it forces WIDE)
template <bool WIDE>
__device__ inline typename VT<WIDE>::T vmConst(int64_t lo, int64_t hi) {
  if constexpr (WIDE) return Int128{(uint64_t)lo, hi};
  else return lo;
}

// CoreTime bitfield (core_time.go): year@50:14 month@46:4 day@41:5
// hour@36:5 minute@30:6 second@24:6
template <bool WIDE>
__device__ inline typename VT<WIDE>::T vmTimeExtract(typename VT<WIDE>::T a,
                                                     int field, bool* ovf) {
  constexpr int kShift[6] = {50, 46, 41, 36, 30, 24};
  constexpr uint64_t kMask[6] = {0x3FFF, 0xF, 0x1F, 0x1F, 0x3F, 0x3F};
  uint64_t bits = VT<WIDE>::toAcc(a).lo;
  return VT<WIDE>::fromI64((int64_t)((bits >> kShift[field]) & kMask[field]),
                           ovf);
}

// builtinAbs*Sig; narrow INT64_MIN -> wide retry via sub overflow
template <bool WIDE>
__device__ inline typename VT<WIDE>::T vmAbs(typename VT<WIDE>::T a,
                                             bool* ovf) {
  if (VT<WIDE>::cmp(a, VT<WIDE>::zero()) < 0)
    a = VT<WIDE>::sub(VT<WIDE>::zero(), a, ovf);
  return a;
}

// builtinGreatest/Least*Sig on two operands (ties keep a)
template <bool WIDE>
__device__ inline typename VT<WIDE>::T vmSelectMinMax(typename VT<WIDE>::T a,
                                                      typename VT<WIDE>::T b,
                                                      bool isMax) {
  int c = VT<WIDE>::cmp(a, b);
  return isMax == (c >= 0) ? a : b;
}

// cast family: round_half_up by `up` = target scale - source scale digits
// (ProduceDecWithSpecifiedTp datum.go:1629; ToInt when the engine lowered
// cast-as-int to target scale 0). p10 = 10^|up|, <= 10^18.
template <bool WIDE>
__device__ inline bool vmRoundScale(typename VT<WIDE>::T a, int up,
                                    int64_t p10, typename VT<WIDE>::T* out,
                                    bool* ovf, uint32_t* err) {
  if (up >= 0) {
    *out = VT<WIDE>::mul(a, VT<WIDE>::fromI64(p10, nullptr), ovf);
    return true;
  }
  __int128 av = vmToI128<WIDE>(a);
  uint64_t div = (uint64_t)p10;
  unsigned __int128 aAbs = (unsigned __int128)(av < 0 ? -av : av);
  unsigned __int128 q = u128DivU64(aAbs, div);
  unsigned __int128 r = aAbs - q * div;
  if (2 * (uint64_t)r >= div) q += 1;  // half away from zero
  return vmFromI128<WIDE>(av < 0 ? -(__int128)q : (__int128)q, out, err);
}

// DecimalDiv (mydecimal.go:1311, doDiv:1168): quotient truncated toward zero
// at the word-granular result scale; e is the exponent with result =
// trunc(a * 10^e / b). Division by zero yields NULL
// (builtin_arithmetic_vec.go:92 handleDivisionByZero): *nul is set and *out
// is left alone.
template <bool WIDE>
__device__ inline bool vmDiv(typename VT<WIDE>::T a, typename VT<WIDE>::T b,
                             int e, typename VT<WIDE>::T* out, bool* nul,
                             uint32_t* err) {
  __int128 bv = vmToI128<WIDE>(b);
  if (bv == 0) {
    *nul = true;
    return true;
  }
  __int128 av = vmToI128<WIDE>(a);
  unsigned __int128 p10 = (unsigned __int128)(uint64_t)kP10(e > 18 ? 18 : e);
  if (e > 18) p10 *= (uint64_t)kP10(e - 18);
  unsigned __int128 aAbs = (unsigned __int128)(av < 0 ? -av : av);
  unsigned __int128 lim =
      ((unsigned __int128)kDivArgMax[e][1] << 64) | kDivArgMax[e][0];
  if (aAbs > lim) {
    atomicOr(err, kErrOverflow);
    return false;
  }
  unsigned __int128 bAbs = (unsigned __int128)(bv < 0 ? -bv : bv);
  unsigned __int128 num = aAbs * p10;
  unsigned __int128 uq = (bAbs >> 64) != 0 ? u128DivBig(num, bAbs)
                                           : u128DivU64(num, (uint64_t)bAbs);
  bool negq = (av < 0) != (bv < 0);
  return vmFromI128<WIDE>(negq ? -(__int128)uq : (__int128)uq, out, err);
}

// One interpreter step for a non-load opcode. OPS is the kernel's opcode set
// (gx_common.h kVmOps*): the division and rounding bodies compile only into
// kernels whose set holds them, and an opcode outside the set -- or one this
// VM does not know -- raises kErrBadDecimal. Returns false on a hard failure
// (error flag already set); arithmetic overflow accumulates in *ovf and the
// caller raises it after its loop.
template <bool WIDE, uint32_t OPS, class VM>
__device__ __attribute__((always_inline)) inline bool vmStep(
    VM& vm, const VmIns& ins, int64_t p10, const int64_t* constLo,
    const int64_t* constHi, uint32_t* err, bool* ovf) {
  using V = VT<WIDE>;
  switch (ins.op) {
    case VM_LOAD_CONST:
      vm.set(ins.dst, vmConst<WIDE>(constLo[ins.a], constHi[ins.a]));
      vm.setNull(ins.dst, false);
      return true;
    case VM_ADD:
      vm.set(ins.dst, V::add(vm.get(ins.a), vm.get(ins.b), ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a) || vm.isNull(ins.b));
      return true;
    case VM_SUB:
      vm.set(ins.dst, V::sub(vm.get(ins.a), vm.get(ins.b), ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a) || vm.isNull(ins.b));
      return true;
    case VM_MUL: {
      bool nul = vm.isNull(ins.a) || vm.isNull(ins.b);
      typename V::T v = V::zero();
      if (!nul) v = V::mul(vm.get(ins.a), vm.get(ins.b), ovf);
      vm.set(ins.dst, v);
      vm.setNull(ins.dst, nul);
      return true;
    }
    case VM_SCALE_UP:
      vm.set(ins.dst, V::mul(vm.get(ins.a), V::fromI64(p10, nullptr), ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a));
      return true;
    case VM_TIME_EXTRACT:
      vm.set(ins.dst, vmTimeExtract<WIDE>(vm.get(ins.a), ins.b, ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a));
      return true;
    case VM_CMP: {
      // comparisons in VALUE context (builtin_compare_vec family): i64
      // 0/1, NULL if either operand is NULL
      int c = V::cmp(vm.get(ins.a), vm.get(ins.b));
      vm.set(ins.dst, V::fromI64(cmpResult(c, ins.c) ? 1 : 0, ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a) || vm.isNull(ins.b));
      return true;
    }
    case VM_IF: {
      // builtinIfSig: NULL/0 cond -> else branch; result = chosen branch
      bool t = !vm.isNull(ins.a) && V::cmp(vm.get(ins.a), V::zero()) != 0;
      vm.set(ins.dst, t ? vm.get(ins.b) : vm.get(ins.c));
      vm.setNull(ins.dst, t ? vm.isNull(ins.b) : vm.isNull(ins.c));
      return true;
    }
    case VM_MAX2:
    case VM_MIN2:
      // NULL if either operand is NULL
      vm.set(ins.dst, vmSelectMinMax<WIDE>(vm.get(ins.a), vm.get(ins.b),
                                           ins.op == VM_MAX2));
      vm.setNull(ins.dst, vm.isNull(ins.a) || vm.isNull(ins.b));
      return true;
    case VM_ABS:
      vm.set(ins.dst, vmAbs<WIDE>(vm.get(ins.a), ovf));
      vm.setNull(ins.dst, vm.isNull(ins.a));
      return true;
    case VM_IFNULL: {
      // builtinIfNullSig: first non-NULL operand; NULL only if both are
      bool an = vm.isNull(ins.a);
      vm.set(ins.dst, an ? vm.get(ins.b) : vm.get(ins.a));
      vm.setNull(ins.dst, an && vm.isNull(ins.b));
      return true;
    }
    case VM_ROUND_SCALE:
      if constexpr ((OPS >> VM_ROUND_SCALE) & 1) {
        // ins.b = target scale, ins.c = source scale
        bool nul = vm.isNull(ins.a);
        typename V::T v = V::zero();
        if (!nul && !vmRoundScale<WIDE>(vm.get(ins.a), ins.b - ins.c, p10, &v,
                                        ovf, err))
          return false;
        vm.set(ins.dst, v);
        vm.setNull(ins.dst, nul);
        return true;
      }
      break;
    case VM_DIV:
      if constexpr ((OPS >> VM_DIV) & 1) {
        bool nul = vm.isNull(ins.a) || vm.isNull(ins.b);
        typename V::T v = V::zero();
        if (!nul && !vmDiv<WIDE>(vm.get(ins.a), vm.get(ins.b), ins.c, &v, &nul,
                                 err))
          return false;
        vm.set(ins.dst, v);
        vm.setNull(ins.dst, nul);
        return true;
      }
      break;
    default:
      break;
  }
  atomicOr(err, kErrBadDecimal);
  return false;
}

}  // namespace gxp
