// GEMM compute-integrity test operands: the content of the A and B matrices
// as a pure function of position. One source of truth for the device
// kernels (gemm_kernels.h) and for host code (mi-stream's operand dump,
// self-test and gold spot-check) — no HIP include, so a plain host compiler
// can use it.
//
//   gemm_operand(seed, which, row, col): which = 0 is A[row = m][col = k],
//   which = 1 is logical B[row = k][col = n].
//
//     x = lo32(row * 0x9E3779B1) ^ lo32(col * 0x85EBCA6B) ^ lo32(seed)
//         ^ lo32(hi32(seed) * 0xC2B2AE35) ^ (which ? 0xA5A5A5A5 : 0)
//     h = lowbias32(x)            (the mixer of memtest's ADDR pattern)
//     value = (int)(h >> 27) - 16   in [-16, 15]
//
// Why the product is known exactly (derived, not measured): operands are
// integers with |v| <= 16, stored as bf16 without rounding (5 significant
// bits of the 8 bf16 has). Every product satisfies |a*b| <= 256, so a
// length-K sum satisfies |sum| <= 256*K. For K <= 32768 that is <= 2^23:
// every partial sum under ANY association is an integer below 2^24, which
// fp32 holds exactly. The correct C is therefore unique whatever order the
// matrix pipe accumulates in, and can be compared bitwise. K <= 32768
// (kGemmExactMaxK) is a hard argument check on the exact path.
//
// The other dense formats (gemm_dense_kernels.h) take the same operands,
// and the same cap. fp16 and fp32 inherit the argument as it stands: the
// operands have at most 5 significant bits, which fp16 (11) and fp32 (24)
// hold without rounding, and accumulation is fp32, so |sum| <= 256*K <=
// 2^23 is exact under any association. int8 accumulates in int32 and fp64
// in fp64: exact while |sum| < 2^31 and <= 2^53, far beyond the cap.
// Every format is therefore compared bitwise.

#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define K3_GEMM_HD __host__ __device__
#else
#define K3_GEMM_HD
#endif

namespace k3samd_kern {

constexpr int kGemmExactMaxK = 32768;  // 256 * K <= 2^23

K3_GEMM_HD inline uint32_t gemm_lowbias32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

K3_GEMM_HD inline int gemm_operand(uint64_t seed, int which, uint32_t row,
                                   uint32_t col) {
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  const uint32_t x = (row * 0x9E3779B1u) ^ (col * 0x85EBCA6Bu) ^ s_lo ^
                     (s_hi * 0xC2B2AE35u) ^ (which ? 0xA5A5A5A5u : 0u);
  return (int)(gemm_lowbias32(x) >> 27) - 16;
}

// bf16 bit pattern of an integer with |v| <= 256 (at most 8 significant
// bits after the leading one is dropped: exact). Integer arithmetic only,
// so host and device agree without any float conversion.
K3_GEMM_HD inline uint16_t gemm_int_to_bf16(int v) {
  if (v == 0) return 0;
  const uint32_t sign = v < 0 ? 0x8000u : 0u;
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0u) ++e;  // floor(log2(a)), <= 8
  const uint32_t mant = ((a << 7) >> e) & 0x7Fu;
  return (uint16_t)(sign | ((uint32_t)(127 + e) << 7) | mant);
}

}  // namespace k3samd_kern
