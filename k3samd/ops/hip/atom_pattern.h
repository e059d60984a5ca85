// Global-atomics integrity test: the value every slot holds before any
// atomic, the operand every contributor applies, and the result, as pure
// functions of (op, seed, slot, contributor). One source of truth for the
// device kernels (atom_kernels.h) and for host code (mi-atomtest's pattern
// dump and self-test, the CPU ops) - no HIP include, so a plain host
// compiler can use it; numpy reproduces it in k3samd/ops/atomtest.py.
//
// A slot is 4 or 8 bytes; every value travels as its bit pattern in a
// uint64_t (the low 32 bits of a 4-byte slot). W contributors w = 0..W-1
// each apply one operand to every slot; the result is the fold of the W
// operands over the init and must not depend on the order of arrival.
//
//   h(op, seed, slot, i) = splitmix64 finaliser of
//       seed ^ slot * 0x9E3779B97F4A7C15 ^ (i + 1) * 0xC2B2AE3D27D4EB4F
//            ^ (op + 1) * 0x165667B19E3779F9            (all mod 2^64)
//   i = 0 is the init, i = w + 1 the operand of contributor w.
//
// Why the result is unique in any order (derived, not measured):
//   add xor (32 / 64)   operands and init are h: wrap-around arithmetic is
//                       associative and commutative.
//   smin smax umin umax the same: min and max are.
//   and or              B = 32 or 64 bits, T = B / 2 tokens. Per slot a
//                       reserved bit r, its neighbour r2 = r + 1, and T
//                       DISTINCT token bits (s + 7 j) mod (B - 2), j < T,
//                       placed past r2 (7 is coprime to 30 and to 62).
//                       Token j belongs to contributor (hi32(h_j) * W) >> 32,
//                       so an operand carries T / W bits on average: the
//                       density follows W. `or`: operand = its tokens,
//                       init = h with the token bits and r cleared and r2
//                       set; `and`: operand = ~tokens, init = h with the
//                       token bits and r set and r2 cleared. Every token
//                       changes its bit, the result is never all-zeros nor
//                       all-ones (bits r, r2), and an operand without a
//                       token is the op's identity.
//   addf32              init an integer in [-2^20, 2^20], operands integers
//                       in [-1024, 1024]: |init| + W * 1024 <= 2^24 for
//                       W <= 4096, so every partial sum in any order is an
//                       integer that fp32 holds exactly. A zero is +0, and
//                       x + (-x) = +0 under round-to-nearest: never -0.
//   addf64              init in [-2^40, 2^40), operands in [-2^30, 2^30):
//                       far below 2^53.
//   pkaddbf16           per 16-bit half: init in [-16, 16], operands +-1:
//                       16 + W <= 2^8 for W <= 240.
//   pkaddf16            per half: init in [-128, 128], operands in [-8, 8]:
//                       128 + 8 W <= 2^11 for W <= 240.
//   minf64 maxf64       odd integers of 52 bits and a sign: integer-valued,
//                       never zero, never NaN, exact in fp64.
//   swap cas (32 / 64)  chain mode: round r moves a slot from v_r to
//                       v_{r+1}, v_i = h(op, seed, slot, i). Here the
//                       "contributor" is the round: atom_operand(.., r, ..)
//                       = v_{r+1} and atom_expected(.., R) = v_R.
//
// atom_shape_ok() states the caps once.

#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define K3_ATOM_HD __host__ __device__
#else
#define K3_ATOM_HD
#endif

namespace k3samd_kern {

enum AtomOp : int {
  kAtomAdd = 0, kAtomAnd, kAtomOr, kAtomXor,
  kAtomSmin, kAtomSmax, kAtomUmin, kAtomUmax,
  kAtomAdd64, kAtomAnd64, kAtomOr64, kAtomXor64,
  kAtomSmin64, kAtomSmax64, kAtomUmin64, kAtomUmax64,
  kAtomAddF32, kAtomAddF64, kAtomMinF64, kAtomMaxF64,
  kAtomPkAddBf16, kAtomPkAddF16,
  kAtomReduceOps,  // the ops above run in reduce mode
  kAtomSwap = kAtomReduceOps, kAtomSwap64, kAtomCas, kAtomCas64,
  kAtomOpCount,
};

// Host only: the command-line and Python name of an op, nullptr if unknown.
inline const char* atom_op_name(int op) {
  static const char* const kNames[kAtomOpCount] = {
      "add",    "and",    "or",     "xor",     "smin",      "smax",
      "umin",   "umax",   "add64",  "and64",   "or64",      "xor64",
      "smin64", "smax64", "umin64", "umax64",  "addf32",    "addf64",
      "minf64", "maxf64", "pkaddbf16", "pkaddf16", "swap",  "swap64",
      "cas",    "cas64"};
  return op >= 0 && op < kAtomOpCount ? kNames[op] : nullptr;
}

constexpr int kAtomMaxContributors = 4096;  // addf32: 2^20 + 4096 * 1024 <= 2^24
constexpr int kAtomMaxPacked = 240;         // bf16: 16 + 240 = 2^8
constexpr int64_t kAtomMaxSlots = 1ll << 30;
constexpr int kAtomTile = 256;  // slots per tile = lanes per workgroup

K3_ATOM_HD constexpr bool atom_op_ok(int op) { return op >= 0 && op < kAtomOpCount; }
K3_ATOM_HD constexpr bool atom_is_chain(int op) { return op >= kAtomSwap; }
K3_ATOM_HD constexpr bool atom_is_int(int op) { return op < kAtomAddF32; }
K3_ATOM_HD constexpr bool atom_is_packed(int op) {
  return op == kAtomPkAddBf16 || op == kAtomPkAddF16;
}
K3_ATOM_HD constexpr bool atom_is64(int op) {
  return (op >= kAtomAdd64 && op <= kAtomUmax64) || op == kAtomAddF64 ||
         op == kAtomMinF64 || op == kAtomMaxF64 || op == kAtomSwap64 ||
         op == kAtomCas64;
}
K3_ATOM_HD constexpr int atom_slot_bytes(int op) { return atom_is64(op) ? 8 : 4; }
// The integer ops' family: kAtomAdd .. kAtomUmax for both widths.
K3_ATOM_HD constexpr int atom_int_base(int op) { return op & 7; }

// Most contributors (chain ops: rounds) an op takes.
K3_ATOM_HD constexpr int atom_w_cap(int op) {
  return atom_is_packed(op) ? kAtomMaxPacked : kAtomMaxContributors;
}

K3_ATOM_HD constexpr bool atom_shape_ok(int op, int64_t slots, int64_t w) {
  return atom_op_ok(op) && slots >= 1 && slots <= kAtomMaxSlots && w >= 1 &&
         w <= atom_w_cap(op);
}

K3_ATOM_HD inline uint64_t atom_mix(int op, uint64_t seed, uint64_t slot,
                                    uint64_t i) {
  uint64_t x = seed ^ (slot * 0x9E3779B97F4A7C15ull) ^
               ((i + 1) * 0xC2B2AE3D27D4EB4Full) ^
               ((uint64_t)(op + 1) * 0x165667B19E3779F9ull);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

K3_ATOM_HD inline uint64_t atom_trunc(int op, uint64_t v) {
  return atom_is64(op) ? v : (v & 0xFFFFFFFFull);
}

// ---- and / or: the token scheme ----

constexpr uint64_t kAtomIdxLayout = 1ull << 40;  // h index of (r, s)
constexpr uint64_t kAtomIdxToken = 1ull << 41;   // + j: h index of token j

struct AtomTokens {
  int bits, r, r2, s;
};

K3_ATOM_HD inline AtomTokens atom_tokens(int op, uint64_t seed, uint64_t slot) {
  const uint64_t h = atom_mix(op, seed, slot, kAtomIdxLayout);
  AtomTokens t;
  t.bits = atom_is64(op) ? 64 : 32;
  t.r = (int)(h & (uint64_t)(t.bits - 1));
  t.r2 = (t.r + 1) & (t.bits - 1);
  t.s = (int)((h >> 32) % (uint64_t)(t.bits - 2));
  return t;
}

K3_ATOM_HD inline uint64_t atom_token_bit(const AtomTokens& t, int j) {
  const int pos = (t.s + 7 * j) % (t.bits - 2);
  return 1ull << ((t.r + 2 + pos) & (t.bits - 1));
}

K3_ATOM_HD inline uint64_t atom_token_union(const AtomTokens& t) {
  uint64_t m = 0;
  for (int j = 0; j < t.bits / 2; ++j) m |= atom_token_bit(t, j);
  return m;
}

// The token bits of contributor w of W.
K3_ATOM_HD inline uint64_t atom_token_mask(int op, uint64_t seed, uint64_t slot,
                                           uint32_t w, uint32_t W) {
  const AtomTokens t = atom_tokens(op, seed, slot);
  uint64_t m = 0;
  for (int j = 0; j < t.bits / 2; ++j) {
    const uint64_t h = atom_mix(op, seed, slot, kAtomIdxToken + (uint64_t)j);
    if ((uint32_t)(((h >> 32) * (uint64_t)W) >> 32) == w)
      m |= atom_token_bit(t, j);
  }
  return m;
}

// ---- float encodings (integer arithmetic, or an exact conversion) ----

// Bits of the 16-bit float with `mant` fraction bits and exponent bias
// `bias` that holds the integer v, |v| <= 2^(mant + 1): exact.
K3_ATOM_HD inline uint32_t atom_int_to_fp16(int v, int mant, int bias) {
  if (v == 0) return 0u;
  const uint32_t sign = v < 0 ? 0x8000u : 0u;
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0u) ++e;
  const uint32_t frac = ((a << mant) >> e) & ((1u << mant) - 1u);
  return sign | ((uint32_t)(bias + e) << mant) | frac;
}

K3_ATOM_HD inline uint64_t atom_f32_bits(int64_t v) {  // |v| <= 2^24
  const float f = (float)v;
  uint32_t b;
  __builtin_memcpy(&b, &f, 4);
  return b;
}

K3_ATOM_HD inline uint64_t atom_f64_bits(int64_t v) {  // |v| <= 2^53
  const double f = (double)v;
  uint64_t b;
  __builtin_memcpy(&b, &f, 8);
  return b;
}

// ---- the integer behind every float value; i = 0 init, i = w + 1 operand ----

K3_ATOM_HD inline int64_t atom_float_int(int op, uint64_t seed, uint64_t slot,
                                         uint64_t i) {
  const uint64_t h = atom_mix(op, seed, slot, i);
  switch (op) {
    case kAtomAddF32:
      return i == 0 ? (int64_t)((h >> 32) % 2097153ull) - 1048576
                    : (int64_t)((h >> 32) % 2049ull) - 1024;
    case kAtomAddF64:
      return i == 0 ? (int64_t)(h >> 23) - (1ll << 40)
                    : (int64_t)(h >> 33) - (1ll << 30);
    default:  // kAtomMinF64, kAtomMaxF64: odd, 52 bits and a sign
      return ((int64_t)h >> 12) | 1;
  }
}

// Half k (0 = low 16 bits) of a packed value.
K3_ATOM_HD inline int atom_packed_int(int op, uint64_t seed, uint64_t slot,
                                      uint64_t i, int k) {
  const uint64_t h = atom_mix(op, seed, slot, i);
  const uint32_t f = (uint32_t)(h >> (16 * k)) & 0xFFFFu;
  if (op == kAtomPkAddBf16)
    return i == 0 ? (int)(f % 33u) - 16 : ((f & 1u) ? 1 : -1);
  return i == 0 ? (int)(f % 257u) - 128 : (int)(f % 17u) - 8;
}

K3_ATOM_HD inline uint64_t atom_packed_bits(int op, int lo, int hi) {
  const int mant = op == kAtomPkAddBf16 ? 7 : 10;
  const int bias = op == kAtomPkAddBf16 ? 127 : 15;
  return atom_int_to_fp16(lo, mant, bias) |
         (atom_int_to_fp16(hi, mant, bias) << 16);
}

// ---- the three functions ----

// v_i of a chain op.
K3_ATOM_HD inline uint64_t atom_chain_value(int op, uint64_t seed,
                                            uint64_t slot, uint64_t i) {
  return atom_trunc(op, atom_mix(op, seed, slot, i));
}

K3_ATOM_HD inline uint64_t atom_init(int op, uint64_t seed, uint64_t slot) {
  if (atom_is_chain(op)) return atom_chain_value(op, seed, slot, 0);
  if (atom_is_packed(op))
    return atom_packed_bits(op, atom_packed_int(op, seed, slot, 0, 0),
                            atom_packed_int(op, seed, slot, 0, 1));
  if (op == kAtomAddF32) return atom_f32_bits(atom_float_int(op, seed, slot, 0));
  if (!atom_is_int(op)) return atom_f64_bits(atom_float_int(op, seed, slot, 0));
  const uint64_t h = atom_mix(op, seed, slot, 0);
  const int base = atom_int_base(op);
  if (base == kAtomAnd || base == kAtomOr) {
    const AtomTokens t = atom_tokens(op, seed, slot);
    const uint64_t u = atom_token_union(t);
    const uint64_t r = 1ull << t.r, r2 = 1ull << t.r2;
    return atom_trunc(op, base == kAtomOr ? ((h & ~u & ~r) | r2)
                                          : ((h | u | r) & ~r2));
  }
  return atom_trunc(op, h);
}

K3_ATOM_HD inline uint64_t atom_operand(int op, uint64_t seed, uint64_t slot,
                                        uint32_t w, uint32_t W) {
  const uint64_t i = (uint64_t)w + 1;
  if (atom_is_chain(op)) return atom_chain_value(op, seed, slot, i);
  if (atom_is_packed(op))
    return atom_packed_bits(op, atom_packed_int(op, seed, slot, i, 0),
                            atom_packed_int(op, seed, slot, i, 1));
  if (op == kAtomAddF32) return atom_f32_bits(atom_float_int(op, seed, slot, i));
  if (!atom_is_int(op)) return atom_f64_bits(atom_float_int(op, seed, slot, i));
  const int base = atom_int_base(op);
  if (base == kAtomAnd || base == kAtomOr) {
    const uint64_t m = atom_token_mask(op, seed, slot, w, W);
    return atom_trunc(op, base == kAtomOr ? m : ~m);
  }
  return atom_trunc(op, atom_mix(op, seed, slot, i));
}

// One step of an integer op's fold, on bit patterns of the op's width.
K3_ATOM_HD inline uint64_t atom_int_step(int op, uint64_t acc, uint64_t v) {
  const bool wide = atom_is64(op);
  switch (atom_int_base(op)) {
    case kAtomAdd: return atom_trunc(op, acc + v);
    case kAtomAnd: return acc & v;
    case kAtomOr: return acc | v;
    case kAtomXor: return acc ^ v;
    case kAtomUmin: return v < acc ? v : acc;
    case kAtomUmax: return v > acc ? v : acc;
    default: {
      const int64_t a = wide ? (int64_t)acc : (int64_t)(int32_t)(uint32_t)acc;
      const int64_t b = wide ? (int64_t)v : (int64_t)(int32_t)(uint32_t)v;
      const bool take = atom_int_base(op) == kAtomSmin ? b < a : b > a;
      return take ? v : acc;
    }
  }
}

// The fold of operands 0..W-1 over the init, skipping contributor `skip`
// (-1: none): a plain loop, no atomic.
K3_ATOM_HD inline uint64_t atom_expected_without(int op, uint64_t seed,
                                                 uint64_t slot, uint32_t W,
                                                 int64_t skip) {
  if (atom_is_chain(op)) return atom_chain_value(op, seed, slot, W);
  if (atom_is_packed(op)) {
    int lo = atom_packed_int(op, seed, slot, 0, 0);
    int hi = atom_packed_int(op, seed, slot, 0, 1);
    for (uint32_t w = 0; w < W; ++w) {
      if ((int64_t)w == skip) continue;
      lo += atom_packed_int(op, seed, slot, (uint64_t)w + 1, 0);
      hi += atom_packed_int(op, seed, slot, (uint64_t)w + 1, 1);
    }
    return atom_packed_bits(op, lo, hi);
  }
  if (!atom_is_int(op)) {
    int64_t acc = atom_float_int(op, seed, slot, 0);
    for (uint32_t w = 0; w < W; ++w) {
      if ((int64_t)w == skip) continue;
      const int64_t v = atom_float_int(op, seed, slot, (uint64_t)w + 1);
      if (op == kAtomMinF64) acc = v < acc ? v : acc;
      else if (op == kAtomMaxF64) acc = v > acc ? v : acc;
      else acc += v;
    }
    return op == kAtomAddF32 ? atom_f32_bits(acc) : atom_f64_bits(acc);
  }
  uint64_t acc = atom_init(op, seed, slot);
  for (uint32_t w = 0; w < W; ++w) {
    if ((int64_t)w == skip) continue;
    acc = atom_int_step(op, acc, atom_operand(op, seed, slot, w, W));
  }
  return acc;
}

K3_ATOM_HD inline uint64_t atom_expected(int op, uint64_t seed, uint64_t slot,
                                         uint32_t W) {
  return atom_expected_without(op, seed, slot, W, -1);
}

// True when applying `operand` can never change a slot (reduce ops): 0 for
// add / or / xor / umax and the float adds, all-ones for and / umin, the
// type's extreme for smin / smax. minf64 / maxf64 have none in the pattern.
K3_ATOM_HD inline bool atom_operand_is_identity(int op, uint64_t operand) {
  if (!atom_is_int(op))
    return op != kAtomMinF64 && op != kAtomMaxF64 && operand == 0;
  const uint64_t ones = atom_trunc(op, ~0ull);
  switch (atom_int_base(op)) {
    case kAtomAnd: case kAtomUmin: return operand == ones;
    case kAtomSmin: return operand == (ones >> 1);
    case kAtomSmax: return operand == (ones ^ (ones >> 1));
    default: return operand == 0;
  }
}

}  // namespace k3samd_kern
