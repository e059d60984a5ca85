// Verified GEMM for the fp16, int8, fp32 and fp64 matrix pipes (gfx950):
// the four dense MFMA datapaths next to bf16 (gemm_kernels.h) and MX
// (mx_gemm_kernels.h), on the tile geometry stated in gemm_kernels.h.
// Shared by the torch extension and mi-stream like the other kernel
// headers. Pure HIP.
//
//   format  operand   C / gold  K-step  MFMA (per K-step and (m, n))
//   fp16    _Float16  fp32      64      2 x v_mfma_f32_16x16x32_f16
//   int8    int8      int32     128     2 x v_mfma_i32_16x16x64_i8
//   fp32    float     fp32      32      8 x v_mfma_f32_16x16x4_f32
//   fp64    double    fp64      16      4 x v_mfma_f64_16x16x4_f64
//
//   gemm_dense_fill_kernel<T>     operands from gemm_pattern.h as T
//   gemm_dense16_nt_kernel<F>     fp16 / int8: 16-byte fragments
//   gemm_dense1_nt_kernel<F>      fp32 / fp64: one element per lane
//   gemm_dense_ref_int_kernel<T>  the product in int32 VALU arithmetic
//
// The K-step is kGemmStepBytes / sizeof(element): one step is 128 bytes of
// every operand row whatever the format, so staging, the LDS image and its
// swizzle are gemm_kernels.h's unchanged. Shape contract M % 128 == N % 128
// == 0, K whole K-steps (gemm_dense_shape_ok; no edge handling).
//
// 16-byte fragments (fp16, int8): gemm_bf16_nt_kernel's structure. One MFMA
// consumes 64 bytes of every row; in MFMA s (0..1) of a step a lane reads
// chunk (s*4 + fq) ^ fsw of its row as one ds_read_b128. Which k each of
// the 16 bytes stands for inside the instruction need not be known: A and
// B are read with the same map, and a common permutation of k leaves the
// product unchanged.
//
// One element per lane (fp32, fp64): a 16x16x4 MFMA takes A[fr][k = fq] and
// B[k = fq][fr], so MFMA s of a step takes element s*4 + fq of row fr, at
// byte (s*4 + fq) * sizeof(T) of the 128-byte row. Its 16-byte chunk index
// goes through the same XOR swizzle, the offset inside the chunk stays:
// one 4- or 8-byte LDS read per fragment (the compiler pairs two fragments
// of a lane into one ds_read2st64_b32 / _b64).
//
// C/D maps. fp16, int8 and fp32 results use the map of every 16x16 MFMA
// (mfma_tile16_index): register j of lane l is row (l>>4)*4 + j, column
// l&15. The f64 form does NOT: register j (a VGPR pair) of lane l is
//   row (l>>4) + 4*j, column l&15
// — found with the identity test (A = I, asymmetric Bt) on MI355X silicon;
// the f32 row formula on it runs clean and puts 3 of every 4 results in the
// wrong row.
//
// fp64 keeps acc[4][4] of 4 doubles = 128 VGPRs under __launch_bounds__
// (256, 2) like the others; no scratch (profiles/r11_gemm_formats.md).

#pragma once

#include "gemm_kernels.h"

namespace k3samd_kern {

// Format ids of the launchers; bf16 (gemm_kernels.h) is not one of them.
constexpr int kGemmFmtFp16 = 1, kGemmFmtInt8 = 2, kGemmFmtFp32 = 3,
              kGemmFmtFp64 = 4;

constexpr bool gemm_dense_fmt_ok(int fmt) {
  return fmt >= kGemmFmtFp16 && fmt <= kGemmFmtFp64;
}
// Bytes of one operand element.
constexpr int gemm_dense_elem_bytes(int fmt) {
  return fmt == kGemmFmtFp16 ? 2 : fmt == kGemmFmtInt8 ? 1
       : fmt == kGemmFmtFp32 ? 4 : 8;
}
// Elements per K-step.
constexpr int gemm_dense_step_k(int fmt) {
  return kGemmStepBytes / gemm_dense_elem_bytes(fmt);
}
constexpr const char* gemm_dense_fmt_name(int fmt) {
  return fmt == kGemmFmtFp16 ? "fp16" : fmt == kGemmFmtInt8 ? "int8"
       : fmt == kGemmFmtFp32 ? "fp32" : "fp64";
}

// True when (fmt, m, n, k) meets the dense kernels' shape contract.
inline bool gemm_dense_shape_ok(int fmt, int64_t m, int64_t n, int64_t k) {
  return gemm_dense_fmt_ok(fmt) && gemm_grid_ok(m, n) && k > 0 &&
         k % gemm_dense_step_k(fmt) == 0 && k <= (1 << 24);
}

// One 16-byte cell = 16 / sizeof(T) consecutive elements of one stored
// row; `cells_per_row` is the stored row length in cells. `which` as for
// gemm_fill_kernel. The generator's integers convert without rounding.
template <typename T>
__global__ void gemm_dense_fill_kernel(u4* __restrict__ p, int64_t n_cells,
                                       int64_t cell_offset, int cells_per_row,
                                       int which, uint64_t seed) {
  constexpr int kPer = 16 / (int)sizeof(T);
  using Cell = __attribute__((ext_vector_type(kPer))) T;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const int64_t cell = cell_offset + i;
  const uint32_t r = (uint32_t)(cell / cells_per_row);
  const uint32_t c0 = (uint32_t)(cell % cells_per_row) * (uint32_t)kPer;
  Cell v;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const uint32_t c = c0 + (uint32_t)e;
    v[e] = (T)(which ? gemm_operand(seed, 1, c, r)
                     : gemm_operand(seed, 0, r, c));
  }
  *reinterpret_cast<Cell*>(p + i) = v;
}

// What differs between the formats of one kernel family: the element, the
// result element, the accumulator, the fragment a lane reads and the MFMA.
// (The types are spelled out so that the host pass, which has no f32x4,
// names the same kernel instances.)
#if K3_HAS_MFMA
#define K3_DENSE_MFMA(builtin) return builtin(a, b, c, 0, 0, 0)
#else
#define K3_DENSE_MFMA(builtin) (void)a; (void)b; return c
#endif
struct GemmFp16 {
  using Elem = _Float16;
  using Out = float;
  using Acc = __attribute__((ext_vector_type(4))) float;
  using Frag = __attribute__((ext_vector_type(8))) _Float16;  // 4 VGPRs
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    K3_DENSE_MFMA(__builtin_amdgcn_mfma_f32_16x16x32_f16);
  }
};
struct GemmInt8 {
  using Elem = int8_t;
  using Out = int;
  using Acc = __attribute__((ext_vector_type(4))) int;
  using Frag = __attribute__((ext_vector_type(4))) int;  // 16 int8
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    K3_DENSE_MFMA(__builtin_amdgcn_mfma_i32_16x16x64_i8);
  }
};
struct GemmFp32 {
  using Elem = float;
  using Out = float;
  using Acc = __attribute__((ext_vector_type(4))) float;
  using Frag = float;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    K3_DENSE_MFMA(__builtin_amdgcn_mfma_f32_16x16x4f32);
  }
};
struct GemmFp64 {
  using Elem = double;
  using Out = double;
  using Acc = __attribute__((ext_vector_type(4))) double;  // 4 VGPR pairs
  using Frag = double;
  static __device__ __forceinline__ Acc mfma(Frag a, Frag b, Acc c) {
    K3_DENSE_MFMA(__builtin_amdgcn_mfma_f64_16x16x4f64);
  }
};
#undef K3_DENSE_MFMA

#if K3_HAS_MFMA
// acc[m][n] is the 16x16 block (m, n) of the wave's sub-tile; register j of
// a lane is row fq * kLaneRows + j * kRegRows of the block, column fr:
// (4, 1) is mfma_tile16_index, (1, 4) the f64 form (top of this file).
template <int kLaneRows, int kRegRows, typename Out, typename Acc>
__device__ __forceinline__ void gemm_dense_store_acc(
    Out* __restrict__ C, int N, const GemmTile& t, const Acc (&acc)[4][4]) {
  Out* c_wave = C + (t.brow + t.wr * 64 + t.fq * kLaneRows) * (int64_t)N +
                t.bcol + t.wc * 64 + t.fr;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        c_wave[(m * 16 + j * kRegRows) * (int64_t)N + n * 16] = acc[m][n][j];
}
#endif

// fp16 / int8. `KB` is the byte length of one stored row.
template <typename F>
__global__ __launch_bounds__(256, 2) void gemm_dense16_nt_kernel(
    const typename F::Elem* __restrict__ A,
    const typename F::Elem* __restrict__ Bt, typename F::Out* __restrict__ C,
    int* __restrict__ where, int KB, int N, int tiles_n) {
#if K3_HAS_MFMA
  using Frag = typename F::Frag;
  using Acc = typename F::Acc;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kGemmTileBytes];
  unsigned char* const lds_a = lds;
  unsigned char* const lds_b = lds + kGemmTileBytes;

  const GemmTile t = gemm_tile(tiles_n);
  if (where != nullptr && threadIdx.x == 0) cu_record_placement(where, t.tile);

  const unsigned char* a_src = gemm_stage_src(A, t.brow, KB, t);
  const unsigned char* b_src = gemm_stage_src(Bt, t.bcol, KB, t);
  const int64_t step32 = 32 * (int64_t)KB;  // 32 rows further down
  const unsigned char* a_rd = lds_a + (t.wr * 64 + t.fr) * kGemmStepBytes;
  const unsigned char* b_rd = lds_b + (t.wc * 64 + t.fr) * kGemmStepBytes;
  Acc acc[4][4] = {};

  for (int kb0 = 0; kb0 < KB; kb0 += kGemmStepBytes) {
    gemm_stage(a_src + kb0, b_src + kb0, step32, lds_a, lds_b, t.wid);
    __syncthreads();  // drains the staging loads (vmcnt(0)), then barrier
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int coff = ((s * 4 + t.fq) ^ t.fsw) << 4;
      Frag af[4], bfr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        af[m] =
            *reinterpret_cast<const Frag*>(a_rd + m * kGemmFragBytes + coff);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        bfr[n] =
            *reinterpret_cast<const Frag*>(b_rd + n * kGemmFragBytes + coff);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = F::mfma(af[m], bfr[n], acc[m][n]);
    }
    __syncthreads();  // everyone is done reading before the next stage
  }
  gemm_dense_store_acc<4, 1>(C, N, t, acc);
#else
  (void)A; (void)Bt; (void)C; (void)where; (void)KB; (void)N; (void)tiles_n;
#endif
}

// fp32 / fp64. `KB` is the byte length of one stored row.
template <typename F>
__global__ __launch_bounds__(256, 2) void gemm_dense1_nt_kernel(
    const typename F::Elem* __restrict__ A,
    const typename F::Elem* __restrict__ Bt, typename F::Out* __restrict__ C,
    int* __restrict__ where, int KB, int N, int tiles_n) {
#if K3_HAS_MFMA
  using Elem = typename F::Elem;
  using Acc = typename F::Acc;
  constexpr int kElem = (int)sizeof(Elem);
  constexpr int kSub = kGemmStepBytes / (4 * kElem);  // MFMAs along k per step
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kGemmTileBytes];
  unsigned char* const lds_a = lds;
  unsigned char* const lds_b = lds + kGemmTileBytes;

  const GemmTile t = gemm_tile(tiles_n);
  if (where != nullptr && threadIdx.x == 0) cu_record_placement(where, t.tile);

  const unsigned char* a_src = gemm_stage_src(A, t.brow, KB, t);
  const unsigned char* b_src = gemm_stage_src(Bt, t.bcol, KB, t);
  const int64_t step32 = 32 * (int64_t)KB;  // 32 rows further down
  const unsigned char* a_rd = lds_a + (t.wr * 64 + t.fr) * kGemmStepBytes;
  const unsigned char* b_rd = lds_b + (t.wc * 64 + t.fr) * kGemmStepBytes;
  Acc acc[4][4] = {};

  for (int kb0 = 0; kb0 < KB; kb0 += kGemmStepBytes) {
    gemm_stage(a_src + kb0, b_src + kb0, step32, lds_a, lds_b, t.wid);
    __syncthreads();  // drains the staging loads (vmcnt(0)), then barrier
#pragma unroll
    for (int s = 0; s < kSub; ++s) {
      // element s*4 + fq of the row: its chunk swizzled, the rest kept
      const int byte = (s * 4 + t.fq) * kElem;
      const int coff = (((byte >> 4) ^ t.fsw) << 4) | (byte & 15);
      Elem af[4], bfr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        af[m] =
            *reinterpret_cast<const Elem*>(a_rd + m * kGemmFragBytes + coff);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        bfr[n] =
            *reinterpret_cast<const Elem*>(b_rd + n * kGemmFragBytes + coff);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = F::mfma(af[m], bfr[n], acc[m][n]);
    }
    __syncthreads();  // everyone is done reading before the next stage
  }
  if constexpr (kElem == 8)
    gemm_dense_store_acc<1, 4>(C, N, t, acc);
  else
    gemm_dense_store_acc<4, 1>(C, N, t, acc);
#else
  (void)A; (void)Bt; (void)C; (void)where; (void)KB; (void)N; (void)tiles_n;
#endif
}

// Four consecutive elements -> four packed int8. Operands on this path
// must be integers in [-128, 127]; the generator's are in [-16, 15].
template <typename T>
__device__ __forceinline__ int gemm_dense_pack4_i8(const T* p) {
  using Quad = __attribute__((ext_vector_type(4))) T;
  const Quad q = *reinterpret_cast<const Quad*>(p);
  return ((int)q[0] & 0xFF) | (((int)q[1] & 0xFF) << 8) |
         (((int)q[2] & 0xFF) << 16) | (int)((uint32_t)(int)q[3] << 24);
}

// Independent reference, the structure of gemm_ref_int_kernel: 64x64
// outputs per 256-thread block, 4x4 per thread, 64 k per step decoded to
// 16 words of four packed int8 per row (a thread decodes word tid & 15 of
// rows tid >> 4 + 16 i), int32 sdot4 accumulation, stored as Out. K is a
// multiple of 16 (the fp64 K-step), so words past K in the last step are
// whole and count as zero. No matrix-pipe instruction.
template <typename T, typename Out>
__global__ __launch_bounds__(256) void gemm_dense_ref_int_kernel(
    const T* __restrict__ A, const T* __restrict__ Bt, Out* __restrict__ gold,
    int K, int N, int tiles_n) {
  __shared__ int as[kGemmRefTile][17], bs[kGemmRefTile][17];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t brow = (int64_t)(blockIdx.x / tiles_n) * kGemmRefTile;
  const int64_t bcol = (int64_t)(blockIdx.x % tiles_n) * kGemmRefTile;

  int acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + tx * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = ty + 16 * i;
      const T* pa = A + (brow + row) * (int64_t)K + k;
      const T* pb = Bt + (bcol + row) * (int64_t)K + k;
      as[row][tx] = k < K ? gemm_dense_pack4_i8(pa) : 0;
      bs[row][tx] = k < K ? gemm_dense_pack4_i8(pb) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int kw = 0; kw < 16; ++kw) gemm_ref_dot_word(as, bs, tx, ty, kw, acc);
    __syncthreads();
  }
  using Out4 = __attribute__((ext_vector_type(4))) Out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Out4 v = {(Out)acc[i][0], (Out)acc[i][1], (Out)acc[i][2],
                    (Out)acc[i][3]};
    *reinterpret_cast<Out4*>(gold + (brow + ty * 4 + i) * (int64_t)N + bcol +
                             tx * 4) = v;
  }
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----
// Every caller guarantees gemm_dense_fmt_ok(fmt).

// `buf` is a stored [rows, cols] matrix of the format's operand type,
// cols a whole number of 16-byte cells.
inline void launch_gemm_dense_fill(hipStream_t stream, int fmt, void* buf,
                                   int which, uint64_t seed, int64_t rows,
                                   int64_t cols) {
  u4* p = static_cast<u4*>(buf);
  const int cells_per_row = (int)(cols * gemm_dense_elem_bytes(fmt) / 16);
  auto kernel = fmt == kGemmFmtFp16   ? gemm_dense_fill_kernel<_Float16>
                : fmt == kGemmFmtInt8 ? gemm_dense_fill_kernel<int8_t>
                : fmt == kGemmFmtFp32 ? gemm_dense_fill_kernel<float>
                                      : gemm_dense_fill_kernel<double>;
  launch_chunked(rows * cells_per_row, [&](int64_t off, int64_t cnt) {
    hipLaunchKernelGGL(kernel, dim3((uint32_t)stream_grid(cnt)),
                       dim3(kThreadsPerBlock), 0, stream, p + off, cnt, off,
                       cells_per_row, which, seed);
  });
}

// Caller guarantees gemm_dense_shape_ok(fmt, m, n, k). `where` may be null.
inline void launch_gemm_dense_nt(hipStream_t stream, int fmt, const void* a,
                                 const void* bt, void* c, void* where,
                                 int64_t m, int64_t n, int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmBM);
  const int kb = (int)(k * gemm_dense_elem_bytes(fmt));
  auto go = [&](auto kernel, auto format) {
    using F = decltype(format);
    hipLaunchKernelGGL(kernel, dim3(g.tiles), dim3(256), 0, stream,
                       static_cast<const typename F::Elem*>(a),
                       static_cast<const typename F::Elem*>(bt),
                       static_cast<typename F::Out*>(c),
                       static_cast<int*>(where), kb, (int)n, g.tiles_n);
  };
  if (fmt == kGemmFmtFp16)
    go(gemm_dense16_nt_kernel<GemmFp16>, GemmFp16{});
  else if (fmt == kGemmFmtInt8)
    go(gemm_dense16_nt_kernel<GemmInt8>, GemmInt8{});
  else if (fmt == kGemmFmtFp32)
    go(gemm_dense1_nt_kernel<GemmFp32>, GemmFp32{});
  else
    go(gemm_dense1_nt_kernel<GemmFp64>, GemmFp64{});
}

// Caller guarantees gemm_dense_shape_ok(fmt, m, n, k) and
// k <= kGemmExactMaxK.
inline void launch_gemm_dense_ref_int(hipStream_t stream, int fmt,
                                      const void* a, const void* bt,
                                      void* gold, int64_t m, int64_t n,
                                      int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmRefTile);
  auto go = [&](auto format) {
    using F = decltype(format);
    using E = typename F::Elem;
    using O = typename F::Out;
    hipLaunchKernelGGL((gemm_dense_ref_int_kernel<E, O>), dim3(g.tiles),
                       dim3(256), 0, stream, static_cast<const E*>(a),
                       static_cast<const E*>(bt), static_cast<O*>(gold), (int)k,
                       (int)n, g.tiles_n);
  };
  if (fmt == kGemmFmtFp16) go(GemmFp16{});
  else if (fmt == kGemmFmtInt8) go(GemmInt8{});
  else if (fmt == kGemmFmtFp32) go(GemmFp32{});
  else go(GemmFp64{});
}

}  // namespace k3samd_kern
