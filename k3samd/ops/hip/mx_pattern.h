// MX (block-scaled fp8 / fp4) compute-integrity test operands: the content
// of the element and scale buffers as a pure function of position. One
// source of truth for the device kernels (mx_gemm_kernels.h) and for host
// code (mi-mxgemm's dumps, self-test and gold spot-check) — no HIP include,
// so a plain host compiler can use it.
//
// Elements share the hash of gemm_pattern.h:
//   h = lowbias32(lo32(row * 0x9E3779B1) ^ lo32(col * 0x85EBCA6B) ^ lo32(seed)
//                 ^ lo32(hi32(seed) * 0xC2B2AE35) ^ (which ? 0xA5A5A5A5 : 0))
//   which = 0 is A[row = m][col = k], which = 1 is logical B[row = k][col = n].
//
//   fp8 e4m3 (OCP e4m3fn, FMT 0): value = gemm_operand() = (int)(h >> 27) - 16,
//     an integer in [-16, 15]; e4m3 has 4 significant bits, so every one is
//     exact. mx_int_to_e4m3() encodes it with integer arithmetic only.
//   fp4 e2m1 (FMT 4): code = h >> 28. Every code is finite: magnitude
//     {0, 0.5, 1, 1.5, 2, 3, 4, 6}[code & 7], bit 3 the sign. Two elements
//     per byte, the low nibble holding the even k.
//
// Scales: one E8M0 byte (2^(byte - 127)) per 32 consecutive k of one STORED
// row (row m of A, row n of Bt):
//   mx_scale(seed, which, r, kblock) = 127 + (top bit of lowbias32 of
//     lo32(r * 0x9E3779B1) ^ lo32(kblock * 0x85EBCA6B) ^ seed terms as above
//     ^ (which ? 0xA5A5A5A5 : 0) ^ 0x3C6EF372)
//   i.e. 127 (x1) or 128 (x2). The salt 0x3C6EF372 keeps the scale of a block
//   uncorrelated with the element that shares its (row, col) numbers.
//
// Stored layouts (the "nt" convention of the bf16 test): A is [M][K] and Bt
// is [N][K], both k-contiguous — K bytes per row for fp8, K/2 for fp4.
// SA is [M][K/32] and SB is [N][K/32], uint8. Bt[n][k] holds logical
// B[k][n] = operand(seed, 1, row = k, col = n).
//
// Why the product is known exactly (derived, not measured):
//   fp8: a scaled element is an integer with |v| <= 16 * 2 = 32, so
//        |a*b| <= 1024 and a length-K sum satisfies |sum| <= 1024 * K, which
//        is <= 2^23 for K <= 8192.
//   fp4: a scaled element is a whole number of halves, at most 6 * 2 = 12
//        = 24 halves. A product is then a whole number of quarters, at most
//        24 * 24 = 576 of them, and 576 * 8192 = 4,718,592 < 2^23 quarters.
//   Every partial sum under ANY association is therefore an integer
//   (multiple of 1/4) below 2^24 units, which fp32 holds exactly: the
//   correct C is unique whatever order the sum is taken in, and is compared
//   bitwise. K <= 8192 (kMxExactMaxK) is a hard argument check.
//
// What this does not cover: how v_mfma_scale_f32_16x16x128_f8f6f4 sums its
// 128 products internally is not documented. That the matrix pipe adds such
// in-bound data exactly is established on silicon by the single-tile tests
// (see profiles/r06_mxgemmtest.md), not by this derivation.

#pragma once

#include <cstdint>

#include "gemm_pattern.h"

namespace k3samd_kern {

constexpr int kMxFmtFp8 = 0, kMxFmtFp4 = 4;  // the instruction's FMT codes
constexpr int kMxExactMaxK = 8192;           // 1024 * K <= 2^23
constexpr int kMxScaleBlock = 32;            // k per E8M0 scale byte
constexpr uint32_t kMxScaleSalt = 0x3C6EF372u;

K3_GEMM_HD inline bool mx_fmt_ok(int fmt) {
  return fmt == kMxFmtFp8 || fmt == kMxFmtFp4;
}

// Stored bytes of `k` elements of one row.
K3_GEMM_HD inline int64_t mx_row_bytes(int fmt, int64_t k) {
  return fmt == kMxFmtFp4 ? k / 2 : k;
}

K3_GEMM_HD inline uint32_t mx_hash(uint64_t seed, int which, uint32_t row,
                                   uint32_t col, uint32_t salt) {
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  return gemm_lowbias32((row * 0x9E3779B1u) ^ (col * 0x85EBCA6Bu) ^ s_lo ^
                        (s_hi * 0xC2B2AE35u) ^ (which ? 0xA5A5A5A5u : 0u) ^
                        salt);
}

// e4m3fn byte of an integer with |v| <= 16 (4 significant bits: exact).
K3_GEMM_HD inline uint8_t mx_int_to_e4m3(int v) {
  if (v == 0) return 0;
  const uint32_t sign = v < 0 ? 0x80u : 0u;
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0u) ++e;  // floor(log2(a)), <= 4
  const uint32_t mant = ((a << 3) >> e) & 7u;
  return (uint8_t)(sign | ((uint32_t)(7 + e) << 3) | mant);
}

// Raw element code at a logical position: the e4m3 byte or the e2m1 nibble.
K3_GEMM_HD inline uint32_t mx_code(int fmt, uint64_t seed, int which,
                                   uint32_t row, uint32_t col) {
  return fmt == kMxFmtFp4 ? mx_hash(seed, which, row, col, 0u) >> 28
                          : mx_int_to_e4m3(gemm_operand(seed, which, row, col));
}

// Integer value of an e4m3fn byte that encodes an integer (fractions are
// truncated; 0x7F / 0xFF, the NaNs, are not handled).
K3_GEMM_HD inline int mx_e4m3_to_int(uint32_t b) {
  const int e = (int)(b >> 3) & 15, m = 8 + (int)(b & 7);
  const int mag = e >= 10 ? m << (e - 10) : e >= 7 ? m >> (10 - e) : 0;
  return (b & 0x80u) ? -mag : mag;
}

// Value of an e2m1 code in units of 1/2: magnitudes {0,1,2,3,4,6,8,12}.
K3_GEMM_HD inline int mx_e2m1_to_halves(uint32_t code) {
  const int e = (int)(code >> 1) & 3, m = (int)(code & 1);
  const int mag = e == 0 ? m : (2 + m) << (e - 1);
  return (code & 8u) ? -mag : mag;
}

// `r` is the stored row: m for A (which = 0), n for Bt (which = 1).
K3_GEMM_HD inline uint8_t mx_scale(uint64_t seed, int which, uint32_t r,
                                   uint32_t kblock) {
  return (uint8_t)(127u + (mx_hash(seed, which, r, kblock, kMxScaleSalt) >> 31));
}

// Unscaled logical element in units of 1 (fp8) or 1/2 (fp4).
K3_GEMM_HD inline int mx_elem_units(int fmt, uint64_t seed, int which,
                                    uint32_t row, uint32_t col) {
  return fmt == kMxFmtFp4
             ? mx_e2m1_to_halves(mx_hash(seed, which, row, col, 0u) >> 28)
             : gemm_operand(seed, which, row, col);
}

}  // namespace k3samd_kern
