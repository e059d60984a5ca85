// Per-CU self-test: geometry, the placement registers (ids, the record
// every kernel writes, the decode), and the VALU signature as a pure
// function. One source of truth for the device kernels (cu_test_kernels.h,
// the GEMM kernels' placement record) and for host code (mi-cutest's
// signature dump and self-test, the torch binding's cu_signature_expected)
// — no HIP include, so a plain host compiler can use it.
//
// Placement. s_getreg HW_ID, gfx9-family layout:
//   WAVE_ID 3:0 | SIMD_ID 5:4 | PIPE_ID 7:6 | CU_ID 11:8 | SH_ID 12 |
//   SE_ID 15:13 | TG_ID 19:16 | VM_ID 23:20 | QUEUE_ID 26:24 |
//   STATE_ID 29:27 | ME_ID 31:30
// cu_key() joins XCC_ID[3:0] with SE, SH and CU (HW_ID bits 15:8) and nothing
// else, so it names one physical CU; cu_simd() is the SIMD inside it. The
// layout is validated on silicon by the coverage conditions of
// tests/test_cutest_gpu.py (distinct keys == CU count, four SIMDs per key),
// see profiles/r07_cutest.md.
//
// VALU signature. One wave of 64 lanes, parameters (seed, rounds); the
// result is one 16-byte cell per lane:
//   d0      bits of the fp32 chain f
//   d1, d2  low and high word of the fp64 chain d
//   d3      integer / cross-lane chain u
// The three datapaths never mix, so the dword index names the failing one.
//
//   H(lane, r, salt) = lowbias32(lo32(lane * 0x9E3779B1) ^ lo32(r * 0x85EBCA6B)
//                        ^ lo32(seed) ^ lo32(hi32(seed) * 0xC2B2AE35) ^ salt)
//   start (r = 0 in H):
//     f = 1 + (H(.., 0xF32A0001) >> 9) * 2^-23                     in [1, 2)
//     d = 1 + H(.., 0xF64A0002) * 2^-32                            in [1, 2)
//     u = H(.., 0x1A7E0003)
//   round r = 0 .. rounds-1:
//     f = fmaf(f, a, b)   a  = 0.5 + (H(.., 0xF32A0011) >> 10) * 2^-24
//                         b  = 1 + (H(.., 0xF32A0012) >> 9) * 2^-23
//     d = fma(d, a', b')  a' = 0.5 + H(.., 0xF64A0021) * 2^-34
//                         b' = 1 + H(.., 0xF64A0022) * 2^-32
//     t = (u64)u * (H(.., 0x1A7E0031) | 1) + H(.., 0x1A7E0032)  (v_mad_u64_u32)
//     u = lo32(t) ^ hi32(t)
//     u = u + sum_i int8(u, i) * int8(q, i),  q = H(.., 0x1A7E0033)   (sdot4,
//         signed bytes, sum mod 2^32 — gemm_dot4_i8's operation)
//     u ^= rotl(u of lane ^ (1 << (r % 6)), 1)    every lane reads the
//         partner's value from BEFORE the exchange
//   a and a' are in [0.5, 0.75), b and b' in [1, 2): from f in [1, 8) follows
//   f*a + b in [1.5, 8), so both chains stay in [1, 8) — no denormal,
//   infinity or NaN ever occurs.
//
// Why the result is compared BITWISE (derived, not measured): IEEE-754 fma
// is correctly rounded, so fmaf/fma give one defined result for given
// operands on every conforming implementation, host or device; the operands
// stay normal, so no flush-to-zero mode can matter; the chains are written
// with the fma builtins only, so contraction settings cannot change them;
// integer arithmetic is mod 2^32. tests/test_cutest_cpu.py pins this header
// and the device against the independent oracle of k3samd/ops/cutest.py.

#pragma once

#include <cstdint>
#include <cstring>

#include "gemm_pattern.h"

#if defined(__HIPCC__)
#define K3_CU_HD __host__ __device__
#else
#define K3_CU_HD
#endif

namespace k3samd_kern {

constexpr int kCuLdsBytes = 163840;              // the whole LDS of one CU
constexpr int kCuLdsCells = kCuLdsBytes / 16;    // 10240 16-byte cells
constexpr int kCuLdsDwords = kCuLdsBytes / 4;    // 40960
constexpr int kCuWgThreads = 256;
constexpr int kCuWaves = 4;
constexpr int kCuWaveLanes = 64;
constexpr int kCuMaxInject = 256;                // inject list rows per launch

// Report cell index of the signature kernel's fifth checked value (the
// cross-wave LDS fold): the lane's cell index with this bit set.
constexpr uint64_t kCuFoldCellBit = 1ull << 40;

// ---- placement: the registers, the record, the decode ----

// s_getreg_b32 operand: id | offset << 6 | (width - 1) << 11, full 32 bits
constexpr int kHwRegHwId = 4 | (31 << 11);
constexpr int kHwRegXccId = 20 | (31 << 11);

#if defined(__HIPCC__)
// where[slot] = {XCC_ID, HW_ID} of the calling wave; the caller picks the
// lane that writes. (__forceinline__ is a HIP-header macro: spelled out.)
__device__ inline __attribute__((always_inline)) void cu_record_placement(
    int* where, int slot) {
  where[2 * slot] = (int)__builtin_amdgcn_s_getreg(kHwRegXccId);
  where[2 * slot + 1] = (int)__builtin_amdgcn_s_getreg(kHwRegHwId);
}
#endif

K3_CU_HD inline uint32_t cu_simd(uint32_t hw_id) { return (hw_id >> 4) & 3u; }
K3_CU_HD inline uint32_t cu_cu(uint32_t hw_id) { return (hw_id >> 8) & 15u; }
K3_CU_HD inline uint32_t cu_sh(uint32_t hw_id) { return (hw_id >> 12) & 1u; }
K3_CU_HD inline uint32_t cu_se(uint32_t hw_id) { return (hw_id >> 13) & 7u; }

// xcc[3:0] : se[2:0] : sh : cu[3:0] — 12 bits, one value per physical CU.
K3_CU_HD inline uint32_t cu_key(uint32_t xcc_id, uint32_t hw_id) {
  return ((xcc_id & 15u) << 8) | ((hw_id >> 8) & 0xFFu);
}

// ---- VALU signature ----

constexpr uint32_t kCuSaltF0 = 0xF32A0001u, kCuSaltD0 = 0xF64A0002u,
                   kCuSaltU0 = 0x1A7E0003u, kCuSaltFa = 0xF32A0011u,
                   kCuSaltFb = 0xF32A0012u, kCuSaltDa = 0xF64A0021u,
                   kCuSaltDb = 0xF64A0022u, kCuSaltUm = 0x1A7E0031u,
                   kCuSaltUc = 0x1A7E0032u, kCuSaltUq = 0x1A7E0033u;

struct CuSigState {
  float f;
  double d;
  uint32_t u;
};

struct CuSigCell {
  uint32_t d[4];
};

K3_CU_HD inline uint32_t cu_hash(uint64_t seed, uint32_t lane, uint32_t r,
                                 uint32_t salt) {
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  return gemm_lowbias32((lane * 0x9E3779B1u) ^ (r * 0x85EBCA6Bu) ^ s_lo ^
                        (s_hi * 0xC2B2AE35u) ^ salt);
}

K3_CU_HD inline float cu_bits_f32(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float f;
  std::memcpy(&f, &b, 4);
  return f;
#endif
}

K3_CU_HD inline double cu_bits_f64(uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)b);
#else
  double d;
  std::memcpy(&d, &b, 8);
  return d;
#endif
}

K3_CU_HD inline uint32_t cu_f32_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
#endif
}

K3_CU_HD inline uint64_t cu_f64_bits(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(d);
#else
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
#endif
}

K3_CU_HD inline uint32_t cu_rotl32(uint32_t v, int r) {  // r in 1..31
  return (v << r) | (v >> (32 - r));
}

// c + a.b over four packed signed bytes, mod 2^32.
K3_CU_HD inline uint32_t cu_dot4_i8(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__) && \
    __has_builtin(__builtin_amdgcn_sdot4)
  return (uint32_t)__builtin_amdgcn_sdot4((int)a, (int)b, (int)c, false);
#else
  for (int i = 0; i < 4; ++i)
    c += (uint32_t)((int)(int8_t)(a >> (8 * i)) * (int)(int8_t)(b >> (8 * i)));
  return c;
#endif
}

K3_CU_HD inline CuSigState cu_sig_init(uint64_t seed, uint32_t lane) {
  CuSigState s;
  s.f = cu_bits_f32(0x3F800000u | (cu_hash(seed, lane, 0, kCuSaltF0) >> 9));
  s.d = cu_bits_f64(0x3FF0000000000000ull |
                    ((uint64_t)cu_hash(seed, lane, 0, kCuSaltD0) << 20));
  s.u = cu_hash(seed, lane, 0, kCuSaltU0);
  return s;
}

// One round of one lane, up to but not including the cross-lane exchange.
K3_CU_HD inline void cu_sig_round(CuSigState& s, uint64_t seed, uint32_t lane,
                                  uint32_t r) {
  const float a =
      cu_bits_f32(0x3F000000u | (cu_hash(seed, lane, r, kCuSaltFa) >> 10));
  const float b =
      cu_bits_f32(0x3F800000u | (cu_hash(seed, lane, r, kCuSaltFb) >> 9));
  s.f = __builtin_fmaf(s.f, a, b);
  const double da = cu_bits_f64(
      0x3FE0000000000000ull | ((uint64_t)cu_hash(seed, lane, r, kCuSaltDa) << 19));
  const double db = cu_bits_f64(
      0x3FF0000000000000ull | ((uint64_t)cu_hash(seed, lane, r, kCuSaltDb) << 20));
  s.d = __builtin_fma(s.d, da, db);
  const uint64_t t =
      (uint64_t)s.u * (uint64_t)(cu_hash(seed, lane, r, kCuSaltUm) | 1u) +
      (uint64_t)cu_hash(seed, lane, r, kCuSaltUc);
  const uint32_t u = (uint32_t)t ^ (uint32_t)(t >> 32);
  s.u = cu_dot4_i8(u, cu_hash(seed, lane, r, kCuSaltUq), u);
}

// The exchange of round r: partner lane and what a lane folds in.
K3_CU_HD inline uint32_t cu_sig_partner(uint32_t lane, uint32_t r) {
  return lane ^ (1u << (r % 6u));
}
K3_CU_HD inline uint32_t cu_sig_exchange(uint32_t own, uint32_t partner_u) {
  return own ^ cu_rotl32(partner_u, 1);
}

K3_CU_HD inline CuSigCell cu_sig_cell(const CuSigState& s) {
  const uint64_t db = cu_f64_bits(s.d);
  CuSigCell c;
  c.d[0] = cu_f32_bits(s.f);
  c.d[1] = (uint32_t)db;
  c.d[2] = (uint32_t)(db >> 32);
  c.d[3] = s.u;
  return c;
}

// The signature kernel's fifth checked value of a lane: the d3 of the four
// waves of a workgroup (all equal to `d3` on a good CU), wave w rotated
// left by w + 1, XORed together.
K3_CU_HD inline uint32_t cu_sig_fold(uint32_t d3) {
  return cu_rotl32(d3, 1) ^ cu_rotl32(d3, 2) ^ cu_rotl32(d3, 3) ^
         cu_rotl32(d3, 4);
}

// Host evaluation of one whole wave: out[lane] for lane 0..63.
inline void cu_signature_wave(uint64_t seed, uint32_t rounds,
                              CuSigCell out[kCuWaveLanes]) {
  CuSigState st[kCuWaveLanes];
  uint32_t before[kCuWaveLanes];
  for (uint32_t l = 0; l < (uint32_t)kCuWaveLanes; ++l)
    st[l] = cu_sig_init(seed, l);
  for (uint32_t r = 0; r < rounds; ++r) {
    for (uint32_t l = 0; l < (uint32_t)kCuWaveLanes; ++l) {
      cu_sig_round(st[l], seed, l, r);
      before[l] = st[l].u;
    }
    for (uint32_t l = 0; l < (uint32_t)kCuWaveLanes; ++l)
      st[l].u = cu_sig_exchange(before[l], before[cu_sig_partner(l, r)]);
  }
  for (uint32_t l = 0; l < (uint32_t)kCuWaveLanes; ++l)
    out[l] = cu_sig_cell(st[l]);
}

}  // namespace k3samd_kern
