// Verified bf16 MFMA GEMM (gfx950): the kernels of the compute-integrity
// test, shared by the torch extension (k3samd_kernels.hip) and the
// standalone payload (native/hipsmoke/mi_stream.hip) the same way
// stream_kernels.h and memtest_kernels.h are. Pure HIP.
//
//   gemm_fill_kernel     operands from gemm_pattern.h as bf16 (A[M,K]
//                        row-major; B stored k-contiguous as Bt[N,K])
//   gemm_bf16_nt_kernel  C[M,N] fp32 = A . Bt^T on the matrix pipes
//   gemm_ref_int_kernel  the same product in int32 VALU arithmetic, no
//                        MFMA: the independent "gold"
//   buf_compare_kernel   C ^ gold per 16-byte cell into the memtest report
//
// With gemm_pattern.h's small-integer operands the fp32 result is exact
// and unique (see the bound there), so C is compared BITWISE against gold.
//
// Tile geometry of gemm_bf16_nt_kernel and mx_gemm_nt_kernel<0|4>
// (mx_gemm_kernels.h), stated once in GemmTile and the gemm_* helpers. It
// is a geometry of BYTES: one K-step is kGemmStepBytes = 128 bytes of every
// operand row = 64 bf16 (kGemmBK), 128 fp8 or 256 fp4. Shape contract
// M % 128 == N % 128 == 0, K whole steps (host-checked; no edge handling):
//   * 128x128 block tile, 256 threads = 2x2 waves, each wave a 64x64
//     sub-tile held as acc[4][4] of f32x4 (16x16 MFMAs: lane l holds row /
//     column l&15 of its fragment, k-group l>>4; C/D as mfma_tile16_index).
//   * Both operand tiles are [128 rows][128 bytes], staged by
//     global_load_lds width 16: one wave instruction writes 1 KiB = 8 whole
//     rows, LDS destination lane-linear; instruction i (0..3) of wave `wid`
//     fills rows (i*4 + wid)*8 .. +7, lane l row +(l>>3), chunk slot l&7.
//   * LDS swizzle: a linear image would put the 16 rows a ds_read_b128
//     lane group reads on two 16-byte slots of the 256-byte bank row (8-way
//     conflict). Chunk c of row r is kept at chunk slot c ^ ((r >> 1) & 7):
//     with r & 1 selecting the half of the bank row, 16 consecutive rows
//     then cover all 16 slots. The XOR is applied to the per-lane SOURCE
//     address of the staging load (i only adds multiples of 32 to the row,
//     so one schunk serves all four) and to the fragment read address (fsw:
//     sub-tile bases are multiples of 16, so it depends on the lane alone)
//     — the same involution on both sides; the LDS destination stays
//     linear, as global_load_lds requires.
//   * One __shared__ array, two plain __syncthreads() per K-step (the
//     first drains the in-flight staging loads before anyone reads).
//   * Flat grid, tile = blockIdx.x, row-major over (M/128, N/128).
//   * where[tile] = {XCC_ID, HW_ID} of the first wave: names the XCD / CU.
// Each kernel keeps its fragment to itself: which chunks a lane reads, the
// MFMA, the MX scale loads. bf16 (v_mfma_f32_16x16x32_bf16, two per step):
// chunk s*4 + (l>>4) for MFMA s, the layout validated by mfma_gemm16_kernel.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cu_pattern.h"
#include "gemm_pattern.h"
#include "memtest_kernels.h"
#include "stream_kernels.h"

namespace k3samd_kern {

constexpr int kGemmBM = 128, kGemmBN = 128;
constexpr int kGemmBK = 64;          // bf16 elements per K-step (host contract)
constexpr int kGemmStepBytes = 128;  // row bytes per K-step, every format
constexpr int kGemmTileBytes = kGemmBM * kGemmStepBytes;  // 16 KiB per operand
constexpr int kGemmFragBytes = 16 * kGemmStepBytes;  // 16 rows: one fragment
constexpr int kGemmRefTile = 64;     // gold: 64x64 per block
static_assert(kGemmBK * 2 == kGemmStepBytes);

// One 16-byte cell = 8 consecutive bf16 of one stored row. `cols8` is the
// stored row length / 8. which = 0: stored [row = m][col = k] holds
// gemm_operand(seed, 0, m, k). which = 1: stored Bt[row = n][col = k]
// holds gemm_operand(seed, 1, k, n).
__global__ void gemm_fill_kernel(u4* __restrict__ p, int64_t n_cells,
                                 int64_t cell_offset, int cols8, int which,
                                 uint64_t seed) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const int64_t cell = cell_offset + i;
  const uint32_t r = (uint32_t)(cell / cols8);
  const uint32_t c0 = (uint32_t)(cell % cols8) * 8u;
  u4 v;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t w = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t c = c0 + 2u * d + h;
      const int val = which ? gemm_operand(seed, 1, c, r)
                            : gemm_operand(seed, 0, r, c);
      w |= (uint32_t)gemm_int_to_bf16(val) << (16 * h);
    }
    v[d] = w;
  }
  p[i] = v;
}

#if K3_HAS_MFMA  // ---- the tile geometry (see the top of this file) ----
// Chunk slot of 16-byte chunk `chunk` of tile row `row`; an involution.
__device__ __forceinline__ int gemm_swizzle(int chunk, int row) {
  return chunk ^ ((row >> 1) & 7);
}

// Where this thread stands in its workgroup's 128x128 tile.
struct GemmTile {
  int wid, tile;       // wave in the workgroup, tile = blockIdx.x
  int64_t brow, bcol;  // first row / column of the tile in C
  int srow, schunk;    // staging: tile row (of instruction 0), SOURCE chunk
  int wr, wc;          // the wave's 64x64 sub-tile
  int fr, fq, fsw;     // fragment row and k-group of this lane; chunk c of
                       // its rows is read at slot c ^ fsw
};

__device__ __forceinline__ GemmTile gemm_tile(int tiles_n) {
  const int tid = threadIdx.x, lane = tid & 63;
  GemmTile t;
  t.wid = tid >> 6, t.tile = blockIdx.x;
  t.brow = (int64_t)(t.tile / tiles_n) * kGemmBM;
  t.bcol = (int64_t)(t.tile % tiles_n) * kGemmBN;
  t.srow = t.wid * 8 + (lane >> 3), t.schunk = gemm_swizzle(lane & 7, t.srow);
  t.wr = t.wid >> 1, t.wc = t.wid & 1;
  t.fr = lane & 15, t.fq = lane >> 4, t.fsw = gemm_swizzle(0, t.fr);
  return t;
}

// This lane's staging source at K-step 0; the tile starts at row `row0`.
__device__ __forceinline__ const unsigned char* gemm_stage_src(
    const void* base, int64_t row0, int row_bytes, const GemmTile& t) {
  return static_cast<const unsigned char*>(base) +
         (row0 + t.srow) * (int64_t)row_bytes + t.schunk * 16;
}

// One K-step of both tiles: gemm_stage_src() advanced to the step.
__device__ __forceinline__ void gemm_stage(
    const unsigned char* a_src, const unsigned char* b_src,
    int64_t step32_bytes, unsigned char* lds_a, unsigned char* lds_b, int wid) {
  using global_ptr = const __attribute__((address_space(1))) void*;
  using lds_ptr = __attribute__((address_space(3))) void*;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dst = (i * 4 + wid) * 1024;  // wave-uniform
    __builtin_amdgcn_global_load_lds((global_ptr)(a_src + i * step32_bytes),
                                     (lds_ptr)(lds_a + dst), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((global_ptr)(b_src + i * step32_bytes),
                                     (lds_ptr)(lds_b + dst), 16, 0, 0);
  }
}

// acc[m][n] is the 16x16 block (m, n) of the wave's sub-tile.
__device__ __forceinline__ void gemm_store_acc(
    float* __restrict__ C, int N, const GemmTile& t, const f32x4 (&acc)[4][4]) {
  float* c_wave = C + (t.brow + t.wr * 64 + t.fq * 4) * (int64_t)N + t.bcol +
                  t.wc * 64 + t.fr;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        c_wave[(m * 16 + j) * (int64_t)N + n * 16] = acc[m][n][j];
}
#endif

// launch bounds (256, 2): with a 512-register budget the compiler keeps the
// accumulators in AGPRs and shuffles ~160 of them per K-step; capped at
// 256 it uses the VGPR form of the MFMA (122 VGPRs, no copies).
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Bt,
    float* __restrict__ C, int* __restrict__ where, int K, int N,
    int tiles_n) {
#if K3_HAS_MFMA
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kGemmTileBytes];
  unsigned char* const lds_a = lds;
  unsigned char* const lds_b = lds + kGemmTileBytes;

  const GemmTile t = gemm_tile(tiles_n);
  if (where != nullptr && threadIdx.x == 0) cu_record_placement(where, t.tile);

  const int KB = 2 * K;  // bytes per stored row
  const unsigned char* a_src = gemm_stage_src(A, t.brow, KB, t);
  const unsigned char* b_src = gemm_stage_src(Bt, t.bcol, KB, t);
  const int64_t step32 = 32 * (int64_t)KB;  // 32 rows further down
  const unsigned char* a_rd = lds_a + (t.wr * 64 + t.fr) * kGemmStepBytes;
  const unsigned char* b_rd = lds_b + (t.wc * 64 + t.fr) * kGemmStepBytes;
  f32x4 acc[4][4] = {};

  for (int k0 = 0; k0 < K; k0 += kGemmBK) {
    gemm_stage(a_src + 2 * k0, b_src + 2 * k0, step32, lds_a, lds_b, t.wid);
    __syncthreads();  // drains the staging loads (vmcnt(0)), then barrier
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int coff = ((s * 4 + t.fq) ^ t.fsw) << 4;
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        af[m] = *reinterpret_cast<const bf16x8*>(a_rd + m * kGemmFragBytes + coff);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        bfr[n] = *reinterpret_cast<const bf16x8*>(b_rd + n * kGemmFragBytes + coff);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[m], bfr[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();  // everyone is done reading before the next stage
  }
  gemm_store_acc(C, N, t, acc);
#else
  (void)A; (void)Bt; (void)C; (void)where; (void)K; (void)N; (void)tiles_n;
#endif
}

// Four consecutive bf16 integers (two dwords) -> four packed int8.
// Operands on this path must be integers in [-128, 127]; the generator's
// are in [-16, 15].
__device__ __forceinline__ int gemm_pack4_i8(uint32_t w0, uint32_t w1) {
  const int e0 = (int)__uint_as_float(w0 << 16);
  const int e1 = (int)__uint_as_float(w0 & 0xFFFF0000u);
  const int e2 = (int)__uint_as_float(w1 << 16);
  const int e3 = (int)__uint_as_float(w1 & 0xFFFF0000u);
  return (e0 & 0xFF) | ((e1 & 0xFF) << 8) | ((e2 & 0xFF) << 16) |
         (int)((uint32_t)e3 << 24);
}

// a.b over four packed int8 plus c, in integer VALU arithmetic.
__device__ __forceinline__ int gemm_dot4_i8(int a, int b, int c) {
#if __has_builtin(__builtin_amdgcn_sdot4) && defined(__gfx950__)
  return __builtin_amdgcn_sdot4(a, b, c, false);
#else
#pragma unroll
  for (int i = 0; i < 4; ++i)
    c += (int)(signed char)(a >> (8 * i)) * (int)(signed char)(b >> (8 * i));
  return c;
#endif
}

// Shared by the gold kernels (this file's and mx_gemm_ref_int_kernel): 64x64
// outputs per block, 4x4 per thread; `as` / `bs` hold 64 k of 64 rows as 16
// words of four packed int8 (+1 pad word against bank conflicts). Word kw:
__device__ __forceinline__ void gemm_ref_dot_word(
    const int (&as)[kGemmRefTile][17], const int (&bs)[kGemmRefTile][17],
    int tx, int ty, int kw, int (&acc)[4][4]) {
  int a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = as[ty * 4 + i][kw];
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = bs[tx * 4 + j][kw];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = gemm_dot4_i8(a[i], b[j], acc[i][j]);
}

// The accumulators count units of 1 / kUnitDenom (a power of two).
template <int kUnitDenom>
__device__ __forceinline__ void gemm_ref_store(
    float* gold, int N, int64_t brow, int64_t bcol, int tx, int ty,
    const int (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f4 v = {(float)acc[i][0], (float)acc[i][1], (float)acc[i][2],
            (float)acc[i][3]};
    if constexpr (kUnitDenom != 1) v *= 1.0f / kUnitDenom;
    *reinterpret_cast<f4*>(gold + (brow + ty * 4 + i) * (int64_t)N + bcol +
                           tx * 4) = v;
  }
}

// Independent reference: operands converted to int8 and packed
// four-along-k in LDS, int32 accumulation. No matrix-pipe instruction.
__global__ __launch_bounds__(256) void gemm_ref_int_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ Bt,
    float* __restrict__ gold, int K, int N, int tiles_n) {
  __shared__ int as[kGemmRefTile][17], bs[kGemmRefTile][17];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t brow = (int64_t)(blockIdx.x / tiles_n) * kGemmRefTile;
  const int64_t bcol = (int64_t)(blockIdx.x % tiles_n) * kGemmRefTile;

  int acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 64) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = tid + 256 * i;  // 512 cells of 8 bf16 per operand tile
      const int row = q >> 3, c = q & 7;
      const u4 va = *reinterpret_cast<const u4*>(
          A + (brow + row) * (int64_t)K + k0 + c * 8);
      const u4 vb = *reinterpret_cast<const u4*>(
          Bt + (bcol + row) * (int64_t)K + k0 + c * 8);
      as[row][2 * c] = gemm_pack4_i8(va.x, va.y);
      as[row][2 * c + 1] = gemm_pack4_i8(va.z, va.w);
      bs[row][2 * c] = gemm_pack4_i8(vb.x, vb.y);
      bs[row][2 * c + 1] = gemm_pack4_i8(vb.z, vb.w);
    }
    __syncthreads();
#pragma unroll
    for (int kw = 0; kw < 16; ++kw) gemm_ref_dot_word(as, bs, tx, ty, kw, acc);
    __syncthreads();
  }
  gemm_ref_store<1>(gold, N, brow, bcol, tx, ty, acc);
}

// Streaming bitwise compare of two equally sized buffers, one 16-byte cell
// per lane. Same contract as mem_verify_kernel: every lane reaches
// mem_account (no early return), zero atomics on a clean pass. With fp32
// data the report's dword index is the linear element index.
__global__ void buf_compare_kernel(const u4* __restrict__ p,
                                   const u4* __restrict__ expected,
                                   int64_t n_cells, uint64_t cell_offset,
                                   unsigned long long* __restrict__ report) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < n_cells;
  const uint64_t c = cell_offset + (uint64_t)i;
  u4 expect = {0u, 0u, 0u, 0u}, diff = {0u, 0u, 0u, 0u};
  if (in_range) {
    expect = __builtin_nontemporal_load(&expected[i]);
    diff = __builtin_nontemporal_load(&p[i]) ^ expect;
  }
  mem_account(report, c, expect, diff);  // all lanes, no early return
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----

// The M / N half of every format's shape contract.
inline bool gemm_grid_ok(int64_t m, int64_t n) {
  return m > 0 && n > 0 && m % kGemmBM == 0 && n % kGemmBN == 0 &&
         m <= (1 << 24) && n <= (1 << 24) &&
         (m / kGemmBM) * (n / kGemmBN) <= (1 << 22);
}

// True when (m, n, k) meets gemm_bf16_nt_kernel's shape contract.
inline bool gemm_shape_ok(int64_t m, int64_t n, int64_t k) {
  return gemm_grid_ok(m, n) && k > 0 && k % kGemmBK == 0 && k <= (1 << 24);
}

// Flat grid of `block` x `block` output tiles over [m, n], row-major.
struct GemmGrid { int tiles_n, tiles; };
inline GemmGrid gemm_grid(int64_t m, int64_t n, int block) {
  const int tiles_n = (int)(n / block);
  return {tiles_n, (int)(m / block) * tiles_n};
}

// `buf` is a stored [rows, cols] bf16 matrix, cols % 8 == 0.
inline void launch_gemm_fill(hipStream_t stream, void* buf, int which,
                             uint64_t seed, int64_t rows, int64_t cols) {
  u4* p = static_cast<u4*>(buf);
  const int cols8 = (int)(cols / 8);
  launch_chunked(rows * cols8, [&](int64_t off, int64_t cnt) {
    hipLaunchKernelGGL(gemm_fill_kernel, dim3((uint32_t)stream_grid(cnt)),
                       dim3(kThreadsPerBlock), 0, stream, p + off, cnt, off,
                       cols8, which, seed);
  });
}

// Caller guarantees gemm_shape_ok(m, n, k). `where` may be null.
inline void launch_gemm_bf16_nt(hipStream_t stream, const void* a,
                                const void* bt, void* c, void* where,
                                int64_t m, int64_t n, int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmBM);
  hipLaunchKernelGGL(gemm_bf16_nt_kernel, dim3(g.tiles), dim3(256), 0, stream,
                     static_cast<const uint16_t*>(a),
                     static_cast<const uint16_t*>(bt), static_cast<float*>(c),
                     static_cast<int*>(where), (int)k, (int)n, g.tiles_n);
}

// Caller guarantees gemm_shape_ok(m, n, k) and k <= kGemmExactMaxK.
inline void launch_gemm_ref_int(hipStream_t stream, const void* a,
                                const void* bt, void* gold, int64_t m,
                                int64_t n, int64_t k) {
  const GemmGrid g = gemm_grid(m, n, kGemmRefTile);
  hipLaunchKernelGGL(gemm_ref_int_kernel, dim3(g.tiles), dim3(256), 0, stream,
                     static_cast<const uint16_t*>(a),
                     static_cast<const uint16_t*>(bt),
                     static_cast<float*>(gold), (int)k, (int)n, g.tiles_n);
}

inline void launch_buf_compare(hipStream_t stream, const void* buf,
                               const void* expected, int64_t n_cells,
                               void* report) {
  const u4* p = static_cast<const u4*>(buf);
  const u4* e = static_cast<const u4*>(expected);
  auto* r = static_cast<unsigned long long*>(report);
  launch_chunked(n_cells, [&](int64_t off, int64_t cnt) {
    hipLaunchKernelGGL(buf_compare_kernel, dim3((uint32_t)stream_grid(cnt)),
                       dim3(kThreadsPerBlock), 0, stream, p + off, e + off,
                       cnt, (uint64_t)off, r);
  });
}

}  // namespace k3samd_kern
