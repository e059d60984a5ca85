// Verified MX (block-scaled fp8 e4m3 / fp4 e2m1) MFMA GEMM (gfx950): the
// kernels of the MX compute-integrity test, shared by the torch extension
// (k3samd_kernels.hip) and the standalone payload
// (native/hipsmoke/mi_mxgemm.hip). Pure HIP.
//
//   mx_gemm16_scaled_kernel  one 16x16x128 tile with per-lane scale
//                            operands: pins the lane -> scale-byte map
//   mx_fill_kernel           elements and E8M0 scales from mx_pattern.h
//   mx_gemm_nt_kernel        C[M,N] fp32 = (A o SA) . (Bt o SB)^T with
//                            v_mfma_scale_f32_16x16x128_f8f6f4
//   mx_gemm_ref_int_kernel   the same product in int32 VALU arithmetic, no
//                            matrix-pipe instruction: the independent "gold"
//
// With mx_pattern.h's operands the fp32 result is exact and unique (see
// the bound there), so C is compared BITWISE against gold by
// buf_compare_kernel (gemm_kernels.h).
//
// Operand layout of the instruction, as found on silicon
// (profiles/r06_mxgemmtest.md) and pinned by mx_gemm16_scaled_kernel's
// tests. Lane l holds row (A) / column (B) l & 15; with q = l >> 4:
//   fp4: its 16 bytes are k = q*32 + j, j = 0..31, low nibble first;
//   fp8: its 32 bytes are two runs of 16: bytes 0..15 are k = q*16 + j,
//        bytes 16..31 are k = 64 + q*16 + j (the instruction works like
//        two K = 64 halves, registers 0-3 then 4-7).
// With opsel s, byte s of lane l's scale register scales row/col l & 15,
// k-block q = k 32q .. 32q+31 — in fp4 the lane's own elements, in fp8 the
// first (q < 2) or second (q >= 2) runs of lane groups 2(q&1), 2(q&1)+1.
// mx_gemm16_kernel (stream_kernels.h) loads fp8 as k = q*32 + j on both
// operands: a consistent permutation of k, invisible with unit scales.
//
// mx_gemm_nt_kernel, shape contract M % 128 == N % 128 == 0, K % 128 == 0
// (fp8) or K % 256 == 0 (fp4), checked on the host; no edge handling.
// One K-step is kGemmStepBytes = 128 BYTES of every row in both formats,
// so tile, staging, swizzle, barriers, placement record and epilogue are
// gemm_kernels.h's GemmTile and gemm_* helpers, described at the top of
// that file. What differs is the fragment: an fp8 lane reads the two chunks
// q and 4 + q (q = lane >> 4) for one MFMA per step; an fp4 lane reads
// chunk s*4 + q into the low four dwords for MFMA s = 0, 1 of the step.
// Scale bytes come straight from global memory, one zero-extended byte
// load per 16-row fragment and k-block, issued ahead of the first barrier
// so that its vmcnt(0) drains them with the staging loads.
//
// Resources (hipcc -O3, gfx950, launch bounds (256, 2)): fp8 162 VGPRs,
// fp4 157 VGPRs, 0 AGPRs, no scratch, 32 KiB LDS, 3 waves per SIMD.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gemm_kernels.h"
#include "mx_pattern.h"

namespace k3samd_kern {

#if K3_HAS_MFMA
using i32x4 = __attribute__((ext_vector_type(4))) int;
#endif

// K elements per K-step of mx_gemm_nt_kernel.
K3_GEMM_HD inline int mx_step_k(int fmt) {
  return fmt == kMxFmtFp4 ? 2 * kGemmStepBytes : kGemmStepBytes;
}

// D[16,16] = (A o SA)[16,128] . (B o SB)[128,16]. A and B are packed as for
// mx_gemm16_kernel (B column-major, k contiguous); SA[16][4] and SB[16][4]
// hold the E8M0 byte of (row or column, k-block of 32).
template <int FMT>  // 0 = fp8 e4m3, 4 = fp4 e2m1
__global__ void mx_gemm16_scaled_kernel(const uint8_t* __restrict__ A,
                                        const uint8_t* __restrict__ SA,
                                        const uint8_t* __restrict__ B,
                                        const uint8_t* __restrict__ SB,
                                        float* __restrict__ D) {
#if K3_HAS_MFMA
  const int l = threadIdx.x;  // one wave
  constexpr int kLaneBytes = FMT == 0 ? 32 : 16;
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
  uint8_t* ab = reinterpret_cast<uint8_t*>(&a);
  uint8_t* bb = reinterpret_cast<uint8_t*>(&b);
#pragma unroll
  for (int j = 0; j < kLaneBytes; ++j) {
    const int k_byte = FMT == 0 ? (j >> 4) * 64 + (l >> 4) * 16 + (j & 15)
                                : (l >> 4) * 16 + j;
    ab[j] = A[(l & 15) * 4 * kLaneBytes + k_byte];
    bb[j] = B[(l & 15) * 4 * kLaneBytes + k_byte];
  }
  // byte 0 = this lane's block scale, bytes 1..3 zero (2^-127): a pipe that
  // took another byte, or another lane's, cannot produce the expected C
  const int sa = SA[(l & 15) * 4 + (l >> 4)];
  const int sb = SB[(l & 15) * 4 + (l >> 4)];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, FMT, FMT,
                                                         0, sa, 0, sb);
  // keep the scale VGPRs alive past the MFMA (see mx_gemm16_kernel)
  __asm__ volatile("" ::"v"(sa), "v"(sb));
#pragma unroll
  for (int r = 0; r < 4; ++r)
    D[((l >> 4) * 4 + r) * 16 + (l & 15)] = acc[r];
#else
  (void)A; (void)SA; (void)B; (void)SB; (void)D;
#endif
}

// One 16-byte cell = 16 (fp8) or 32 (fp4) consecutive k of one stored row;
// `cells_per_row` is the row's byte length / 16. The lane whose cell opens
// a block of 32 k also writes that block's scale byte. which = 0: stored
// [r = m][k] holds operand (row m, col k); which = 1: stored Bt[r = n][k]
// holds operand (row k, col n).
__global__ void mx_fill_kernel(u4* __restrict__ elems,
                               uint8_t* __restrict__ scales, int64_t n_cells,
                               int64_t cell_offset, int cells_per_row, int fmt,
                               int which, uint64_t seed) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const int64_t cell = cell_offset + i;
  const uint32_t r = (uint32_t)(cell / cells_per_row);
  const uint32_t c = (uint32_t)(cell % cells_per_row);
  const bool fp4 = fmt == kMxFmtFp4;
  const uint32_t k0 = c * (fp4 ? 32u : 16u);
  auto code = [&](uint32_t k) {
    return which ? mx_code(fmt, seed, 1, k, r) : mx_code(fmt, seed, 0, r, k);
  };
  u4 v;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t byte = 4u * d + b;
      const uint32_t x = fp4 ? code(k0 + 2 * byte) | (code(k0 + 2 * byte + 1) << 4)
                             : code(k0 + byte);
      w |= x << (8 * b);
    }
    v[d] = w;
  }
  elems[i] = v;
  if (k0 % kMxScaleBlock == 0) {
    const uint32_t blocks_per_row = (uint32_t)cells_per_row / (fp4 ? 1u : 2u);
    const uint32_t kblock = k0 / kMxScaleBlock;
    scales[(int64_t)r * blocks_per_row + kblock] =
        mx_scale(seed, which, r, kblock);
  }
}

// `KB` is the byte length of one stored row (K for fp8, K / 2 for fp4).
template <int FMT>
__global__ __launch_bounds__(256, 2) void mx_gemm_nt_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ SA,
    const uint8_t* __restrict__ Bt, const uint8_t* __restrict__ SB,
    float* __restrict__ C, int* __restrict__ where, int KB, int N,
    int tiles_n) {
#if K3_HAS_MFMA
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kGemmTileBytes];
  unsigned char* const lds_a = lds;
  unsigned char* const lds_b = lds + kGemmTileBytes;
  constexpr int kSub = FMT == 0 ? 1 : 2;  // MFMAs along k per K-step

  const GemmTile t = gemm_tile(tiles_n);
  if (where != nullptr && threadIdx.x == 0) cu_record_placement(where, t.tile);

  const unsigned char* a_src = gemm_stage_src(A, t.brow, KB, t);
  const unsigned char* b_src = gemm_stage_src(Bt, t.bcol, KB, t);
  const int64_t step32 = 32 * (int64_t)KB;  // 32 rows further down
  const unsigned char* a_rd = lds_a + (t.wr * 64 + t.fr) * kGemmStepBytes;
  const unsigned char* b_rd = lds_b + (t.wc * 64 + t.fr) * kGemmStepBytes;

  // Scales: this lane's fragment m (n) is row brow + wr*64 + m*16 + fr,
  // and in MFMA s of a step it holds k-block step * 4 * kSub + s * 4 + fq.
  const int SK = KB / (kMxScaleBlock / (FMT == 0 ? 1 : 2));  // K / 32
  const uint8_t* sa_src = SA + (t.brow + t.wr * 64 + t.fr) * (int64_t)SK + t.fq;
  const uint8_t* sb_src = SB + (t.bcol + t.wc * 64 + t.fr) * (int64_t)SK + t.fq;
  const int64_t sstep16 = 16 * (int64_t)SK;  // 16 rows further down
  f32x4 acc[4][4] = {};

  for (int kb0 = 0; kb0 < KB; kb0 += kGemmStepBytes) {
    gemm_stage(a_src + kb0, b_src + kb0, step32, lds_a, lds_b, t.wid);
    // byte 0 = the scale, bytes 1..3 zero; opsel 0 selects byte 0
    const int sblk = kb0 / kGemmStepBytes * 4 * kSub;
    int sa[kSub][4], sb[kSub][4];
#pragma unroll
    for (int s = 0; s < kSub; ++s)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        sa[s][m] = sa_src[m * sstep16 + sblk + s * 4];
        sb[s][m] = sb_src[m * sstep16 + sblk + s * 4];
      }
    __syncthreads();  // drains staging and scale loads (vmcnt(0)), barrier
#pragma unroll
    for (int s = 0; s < kSub; ++s) {
      i32x8 af[4], bfr[4];
      const i32x4 zero = {0, 0, 0, 0};
      if constexpr (FMT == 0) {
        const int c0 = (t.fq ^ t.fsw) << 4, c1 = ((4 + t.fq) ^ t.fsw) << 4;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const unsigned char* p = a_rd + m * kGemmFragBytes;
          af[m] = __builtin_shufflevector(
              *reinterpret_cast<const i32x4*>(p + c0),
              *reinterpret_cast<const i32x4*>(p + c1), 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const unsigned char* p = b_rd + n * kGemmFragBytes;
          bfr[n] = __builtin_shufflevector(
              *reinterpret_cast<const i32x4*>(p + c0),
              *reinterpret_cast<const i32x4*>(p + c1), 0, 1, 2, 3, 4, 5, 6, 7);
        }
      } else {
        const int coff = ((s * 4 + t.fq) ^ t.fsw) << 4;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          af[m] = __builtin_shufflevector(
              *reinterpret_cast<const i32x4*>(a_rd + m * kGemmFragBytes + coff),
              zero, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          bfr[n] = __builtin_shufflevector(
              *reinterpret_cast<const i32x4*>(b_rd + n * kGemmFragBytes + coff),
              zero, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              af[m], bfr[n], acc[m][n], FMT, FMT, 0, sa[s][m], 0, sb[s][n]);
      // keep the scale VGPRs alive past the MFMAs (see mx_gemm16_kernel)
#pragma unroll
      for (int m = 0; m < 4; ++m)
        __asm__ volatile("" ::"v"(sa[s][m]), "v"(sb[s][m]));
    }
    __syncthreads();  // everyone is done reading before the next stage
  }
  gemm_store_acc(C, N, t, acc);
#else
  (void)A; (void)SA; (void)Bt; (void)SB; (void)C; (void)where; (void)KB;
  (void)N; (void)tiles_n;
#endif
}

// Four consecutive elements -> four packed int8, each multiplied by
// 2^shift: `w` holds four e4m3 bytes (units of 1) or, in its low 16 bits,
// four e2m1 nibbles (units of 1/2). Elements must decode to integers and
// stay within int8 after the shift; the generator's do (|v| <= 32 / 24).
template <int FMT>
__device__ __forceinline__ int mx_pack4_i8(uint32_t w, int shift) {
  int out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int v = FMT == 0 ? mx_e4m3_to_int((w >> (8 * e)) & 0xFFu)
                           : mx_e2m1_to_halves((w >> (4 * e)) & 0xFu);
    out |= ((v * (1 << shift)) & 0xFF) << (8 * e);
  }
  return out;
}

// Independent reference, the structure of gemm_ref_int_kernel: 64x64
// outputs per 256-thread block, 4x4 per thread, 64 k per step. Each thread
// decodes 16 consecutive k of one row of each operand with integer
// operations, applies the block's scale as a left shift by (scale - 127)
// (scales must be >= 127) and stores them packed four-along-k in LDS;
// int32 sdot4 accumulation. No matrix-pipe instruction. The accumulator
// counts units of 1 (fp8) or 1/4 (fp4: the product of two half-unit values).
template <int FMT>
__global__ __launch_bounds__(256) void mx_gemm_ref_int_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ SA,
    const uint8_t* __restrict__ Bt, const uint8_t* __restrict__ SB,
    float* __restrict__ gold, int K, int N, int tiles_n) {
  __shared__ int as[kGemmRefTile][17], bs[kGemmRefTile][17];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t brow = (int64_t)(blockIdx.x / tiles_n) * kGemmRefTile;
  const int64_t bcol = (int64_t)(blockIdx.x % tiles_n) * kGemmRefTile;
  const int SK = K / kMxScaleBlock;
  const int row = tid >> 2, c = tid & 3;  // this thread's 16 k: c*16 .. +15

  int acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + c * 16;
    const int sha = (int)SA[(brow + row) * (int64_t)SK + k / kMxScaleBlock] - 127;
    const int shb = (int)SB[(bcol + row) * (int64_t)SK + k / kMxScaleBlock] - 127;
    if constexpr (FMT == 0) {
      const u4 va = *reinterpret_cast<const u4*>(A + (brow + row) * (int64_t)K + k);
      const u4 vb = *reinterpret_cast<const u4*>(Bt + (bcol + row) * (int64_t)K + k);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        as[row][4 * c + d] = mx_pack4_i8<0>(va[d], sha);
        bs[row][4 * c + d] = mx_pack4_i8<0>(vb[d], shb);
      }
    } else {
      const uint2 va = *reinterpret_cast<const uint2*>(
          A + ((brow + row) * (int64_t)K + k) / 2);
      const uint2 vb = *reinterpret_cast<const uint2*>(
          Bt + ((bcol + row) * (int64_t)K + k) / 2);
      as[row][4 * c + 0] = mx_pack4_i8<4>(va.x & 0xFFFFu, sha);
      as[row][4 * c + 1] = mx_pack4_i8<4>(va.x >> 16, sha);
      as[row][4 * c + 2] = mx_pack4_i8<4>(va.y & 0xFFFFu, sha);
      as[row][4 * c + 3] = mx_pack4_i8<4>(va.y >> 16, sha);
      bs[row][4 * c + 0] = mx_pack4_i8<4>(vb.x & 0xFFFFu, shb);
      bs[row][4 * c + 1] = mx_pack4_i8<4>(vb.x >> 16, shb);
      bs[row][4 * c + 2] = mx_pack4_i8<4>(vb.y & 0xFFFFu, shb);
      bs[row][4 * c + 3] = mx_pack4_i8<4>(vb.y >> 16, shb);
    }
    __syncthreads();
#pragma unroll
    for (int kw = 0; kw < 16; ++kw) gemm_ref_dot_word(as, bs, tx, ty, kw, acc);
    __syncthreads();
  }
  gemm_ref_store<FMT == 0 ? 1 : 4>(gold, N, brow, bcol, tx, ty, acc);
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----

// True when (fmt, m, n, k) meets mx_gemm_nt_kernel's shape contract.
inline bool mx_shape_ok(int fmt, int64_t m, int64_t n, int64_t k) {
  return mx_fmt_ok(fmt) && gemm_grid_ok(m, n) && k > 0 &&
         k % mx_step_k(fmt) == 0 && k <= (1 << 24);
}

// `elems` is a stored [rows][k] element matrix (mx_row_bytes(fmt, k) bytes
// per row), `scales` its [rows][k / 32] E8M0 bytes; k % 32 == 0.
inline void launch_mx_fill(hipStream_t stream, void* elems, void* scales,
                           int which, uint64_t seed, int64_t rows, int64_t k,
                           int fmt) {
  u4* p = static_cast<u4*>(elems);
  const int cells_per_row = (int)(mx_row_bytes(fmt, k) / 16);
  launch_chunked(rows * cells_per_row, [&](int64_t off, int64_t cnt) {
    hipLaunchKernelGGL(mx_fill_kernel, dim3((uint32_t)stream_grid(cnt)),
                       dim3(kThreadsPerBlock), 0, stream, p + off,
                       static_cast<uint8_t*>(scales), cnt, off, cells_per_row,
                       fmt, which, seed);
  });
}

// Caller guarantees mx_fmt_ok(fmt). All buffers as for mx_gemm16_scaled_kernel.
inline void launch_mx_gemm16_scaled(hipStream_t stream, int fmt, const void* a,
                                    const void* sa, const void* b,
                                    const void* sb, void* d) {
  auto kernel = fmt == kMxFmtFp8 ? mx_gemm16_scaled_kernel<0>
                                 : mx_gemm16_scaled_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, stream,
                     static_cast<const uint8_t*>(a),
                     static_cast<const uint8_t*>(sa),
                     static_cast<const uint8_t*>(b),
                     static_cast<const uint8_t*>(sb), static_cast<float*>(d));
}

// Caller guarantees mx_shape_ok(fmt, m, n, k). `where` may be null.
inline void launch_mx_gemm_nt(hipStream_t stream, int fmt, const void* a,
                              const void* sa, const void* bt, const void* sb,
                              void* c, void* where, int64_t m, int64_t n,
                              int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmBM);
  auto kernel = fmt == kMxFmtFp8 ? mx_gemm_nt_kernel<0> : mx_gemm_nt_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3(g.tiles), dim3(256), 0, stream,
                     static_cast<const uint8_t*>(a),
                     static_cast<const uint8_t*>(sa),
                     static_cast<const uint8_t*>(bt),
                     static_cast<const uint8_t*>(sb), static_cast<float*>(c),
                     static_cast<int*>(where), (int)mx_row_bytes(fmt, k),
                     (int)n, g.tiles_n);
}

// Caller guarantees mx_shape_ok(fmt, m, n, k) and k <= kMxExactMaxK.
inline void launch_mx_gemm_ref_int(hipStream_t stream, int fmt, const void* a,
                                   const void* sa, const void* bt,
                                   const void* sb, void* gold, int64_t m,
                                   int64_t n, int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmRefTile);
  auto kernel = fmt == kMxFmtFp8 ? mx_gemm_ref_int_kernel<0>
                                 : mx_gemm_ref_int_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3(g.tiles), dim3(256), 0, stream,
                     static_cast<const uint8_t*>(a),
                     static_cast<const uint8_t*>(sa),
                     static_cast<const uint8_t*>(bt),
                     static_cast<const uint8_t*>(sb),
                     static_cast<float*>(gold), (int)k, (int)n, g.tiles_n);
}

}  // namespace k3samd_kern
