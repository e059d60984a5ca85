// Per-CU self-test kernels (gfx950): an LDS march and a VALU signature,
// shared by the torch extension (k3samd_kernels.hip) and the standalone
// payload (native/hipsmoke/mi_cutest.hip) the same way the other kernel
// headers are. Pure HIP, plain C++ and builtins only.
//
// Geometry of both: one workgroup = 256 threads = 4 waves, and a static
// __shared__ array of the full 163,840 B, so at most ONE workgroup is
// resident per CU and a launch of at least multiProcessorCount workgroups
// on an idle device puts one on every CU. Compiler remarks
// (-Rpass-analysis=kernel-resource-usage, gfx950):
//   cu_lds_march_kernel       LDS Size 163840 bytes/block, Occupancy 1
//   cu_valu_signature_kernel  LDS Size 163840 bytes/block, Occupancy 1
// (register counts: profiles/r07_cutest.md).
//
// Both account miscompares through mem_account() into the memtest report
// (int64[56]); a clean run issues no atomic.
//
// cu_lds_march_kernel — global cell index c = wg * kCuLdsCells + cell with
// memtest_cell() unchanged, so every CU's LDS holds address-unique data that
// differs from every other CU's. Per pass p, s = seed + p:
//   phase 0 fill ADDR | 1 verify ADDR, write ~ADDR | 2 verify ~ADDR, write
//   WALK | 3 verify WALK, write CHECKER | 4 verify CHECKER
// with __syncthreads() between phases. In phase ph thread t handles cells
// ((t + 64*ph) & 255) + 256*j, j = 0..39, so what one wave (SIMD) wrote is
// verified by another; 10240 = 40 * 256, no ragged tail. 16-byte accesses.
// Report dword g: wg = g / 40960, LDS byte offset 4 * (g % 40960).
// where[wg] = {XCC_ID, HW_ID} of the workgroup's first wave.
//   stop_after (0..4): the LAST pass ends after that phase; `dump`
//     ([wgs][40960] dwords, optional) receives the LDS content at the end —
//     nothing outside the kernel can read LDS, so this is how the fill path
//     is tested.
//   inject rows (wg, lds_dword, xor_mask, phase 0..3), optional: applied in
//     pass 0 by one thread after that phase's write and barrier, followed by
//     another barrier. Planted corruption in the kernel's own scratch is the
//     only way to drill an LDS detector.
//
// cu_valu_signature_kernel — every wave runs cu_pattern.h's signature for
// `rounds` rounds and compares its 64 cells with expected[64][4] (host
// computed), cell index c = (wg*4 + wave)*64 + lane: g = 4c + k names the
// workgroup (-> CU), wave (-> SIMD via where), lane and datapath k.
// where[wg*4 + wave] = {XCC_ID, HW_ID} of that wave.
//   The LDS array is used for real: each lane stores its d3 at cell
//   (wave*64 + lane) * 40 — the 256 slots span the whole 160 KiB — and after
//   a barrier every wave folds the four waves' d3 of its lane
//   (cu_sig_fold) into a fifth checked value, accounted at cell index
//   kCuFoldCellBit | c, dword 0.
//   inject rows (wg, wave, lane, k, xor_mask), optional: XORed into the
//   computed cell (k = 0..3) or the fold (k = 4) before the compare; the
//   fold itself is taken from the values before injection.
//   sig_out ([wgs*4*64][4] dwords, optional) receives every wave's cells as
//   compared.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cu_pattern.h"
#include "memtest_kernels.h"

namespace k3samd_kern {

constexpr int kCuCellsPerThread = kCuLdsCells / kCuWgThreads;  // 40
constexpr int kCuFoldStride = kCuCellsPerThread;  // cells between fold slots

// What the LDS holds after phase `ph` (0..3) wrote it.
__device__ __forceinline__ MemSpec cu_lds_spec(int ph, uint64_t s) {
  return ph == 0   ? MemSpec{s, kMemPatternAddr, 0}
         : ph == 1 ? MemSpec{s, kMemPatternAddr, 1}
         : ph == 2 ? MemSpec{s, kMemPatternWalk, 0}
                   : MemSpec{s, kMemPatternChecker, 0};
}

template <int PH>
__device__ __forceinline__ void cu_lds_phase(u4* lds, uint64_t base, uint64_t s,
                                             unsigned long long* report) {
  const int t0 = ((int)threadIdx.x + 64 * PH) & (kCuWgThreads - 1);
#pragma unroll 4
  for (int j = 0; j < kCuCellsPerThread; ++j) {
    const int cell = t0 + kCuWgThreads * j;
    const uint64_t c = base + (uint64_t)cell;
    if constexpr (PH >= 1) {
      const u4 expect = mem_expected(cu_lds_spec(PH - 1, s), c);
      const u4 diff = lds[cell] ^ expect;
      if constexpr (PH <= 3) lds[cell] = mem_expected(cu_lds_spec(PH, s), c);
      mem_account(report, c, expect, diff);  // whole wave, no early return
    } else {
      lds[cell] = mem_expected(cu_lds_spec(0, s), c);
    }
  }
}

__global__ __launch_bounds__(kCuWgThreads) void cu_lds_march_kernel(
    unsigned long long* __restrict__ report, int* __restrict__ where,
    uint64_t seed, int passes, int stop_after,
    const long long* __restrict__ inject, int n_inject, u4* __restrict__ dump) {
  __shared__ u4 lds[kCuLdsCells];
  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  const uint64_t base = (uint64_t)wg * kCuLdsCells;

  if (tid == 0) cu_record_placement(where, wg);

  // after the write of phase `ph` of pass 0 (workgroup-uniform control flow)
  auto plant = [&](int ph) {
    if (n_inject == 0) return;
    if (tid == 0) {
      uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
      for (int i = 0; i < n_inject; ++i) {
        const long long* row = inject + 4 * i;
        if (row[0] == wg && row[3] == ph &&
            (unsigned long long)row[1] < (unsigned long long)kCuLdsDwords)
          l32[row[1]] ^= (uint32_t)row[2];
      }
    }
    __syncthreads();
  };

  for (int p = 0; p < passes; ++p) {
    const uint64_t s = seed + (uint64_t)p;
    const int stop = p == passes - 1 ? stop_after : 4;
    const bool first = p == 0;
    cu_lds_phase<0>(lds, base, s, report);
    __syncthreads();
    if (first) plant(0);
    if (stop < 1) break;
    cu_lds_phase<1>(lds, base, s, report);
    __syncthreads();
    if (first) plant(1);
    if (stop < 2) break;
    cu_lds_phase<2>(lds, base, s, report);
    __syncthreads();
    if (first) plant(2);
    if (stop < 3) break;
    cu_lds_phase<3>(lds, base, s, report);
    __syncthreads();
    if (first) plant(3);
    if (stop < 4) break;
    cu_lds_phase<4>(lds, base, s, report);
    __syncthreads();  // phase 0 of the next pass rewrites other waves' cells
  }

  if (dump != nullptr) {
    for (int j = 0; j < kCuCellsPerThread; ++j) {
      const int cell = tid + kCuWgThreads * j;
      dump[base + (uint64_t)cell] = lds[cell];
    }
  }
}

__global__ __launch_bounds__(kCuWgThreads) void cu_valu_signature_kernel(
    unsigned long long* __restrict__ report, int* __restrict__ where,
    uint64_t seed, int rounds, const u4* __restrict__ expected,
    u4* __restrict__ sig_out, const long long* __restrict__ inject,
    int n_inject) {
  __shared__ u4 lds[kCuLdsCells];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = blockIdx.x;
  const int slot = wg * kCuWaves + wave;

  if (lane == 0) cu_record_placement(where, slot);

  CuSigState st = cu_sig_init(seed, (uint32_t)lane);
  for (int r = 0; r < rounds; ++r) {
    cu_sig_round(st, seed, (uint32_t)lane, (uint32_t)r);
    // every lane is active: the partner's pre-exchange value
    const uint32_t other =
        (uint32_t)__shfl_xor((int)st.u, 1 << ((uint32_t)r % 6u), 64);
    st.u = cu_sig_exchange(st.u, other);
  }
  const CuSigCell mine = cu_sig_cell(st);
  u4 cell = {mine.d[0], mine.d[1], mine.d[2], mine.d[3]};

  // cross-wave fold through LDS slots spread over the whole array
  lds[tid * kCuFoldStride].x = cell.w;
  __syncthreads();
  uint32_t fold = 0;
#pragma unroll
  for (int w = 0; w < kCuWaves; ++w)
    fold ^= cu_rotl32(lds[(w * 64 + lane) * kCuFoldStride].x, w + 1);

  for (int i = 0; i < n_inject; ++i) {
    const long long* row = inject + 5 * i;
    if (row[0] == wg && row[1] == wave && row[2] == lane) {
      const uint32_t mask = (uint32_t)row[4];
      const int k = (int)row[3];
      if (k == 4) fold ^= mask;
      else if (k >= 0 && k < 4) cell[k] ^= mask;
    }
  }

  const uint64_t c = (uint64_t)slot * 64u + (uint64_t)lane;
  if (sig_out != nullptr) sig_out[c] = cell;
  const u4 expect = expected[lane];
  mem_account(report, c, expect, cell ^ expect);
  const u4 fold_expect = {cu_sig_fold(expect.w), 0u, 0u, 0u};
  const u4 fold_diff = {fold ^ fold_expect.x, 0u, 0u, 0u};
  mem_account(report, kCuFoldCellBit | c, fold_expect, fold_diff);
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----

// True when `wgs` is a grid size the launchers accept: report indices stay
// far below kCuFoldCellBit.
inline bool cu_grid_ok(int64_t wgs) { return wgs >= 1 && wgs <= (1 << 20); }

// Caller guarantees cu_grid_ok(wgs), passes >= 1, 0 <= stop_after <= 4, and
// every inject row in range (wg < wgs, dword < 40960, phase 0..3). `where`
// is int[wgs][2]; `inject` (device, n_inject rows of 4 int64) and `dump`
// (device, wgs * 163840 B) may be null.
inline void launch_cu_lds_march(hipStream_t stream, void* report, void* where,
                                int64_t wgs, uint64_t seed, int passes,
                                int stop_after, const void* inject,
                                int n_inject, void* dump) {
  hipLaunchKernelGGL(cu_lds_march_kernel, dim3((uint32_t)wgs),
                     dim3(kCuWgThreads), 0, stream,
                     static_cast<unsigned long long*>(report),
                     static_cast<int*>(where), seed, passes, stop_after,
                     static_cast<const long long*>(inject), n_inject,
                     static_cast<u4*>(dump));
}

// Caller guarantees cu_grid_ok(wgs), rounds >= 1 and every inject row in
// range (wg < wgs, wave < 4, lane < 64, k <= 4). `where` is int[wgs*4][2],
// `expected` 64 cells on the device; `sig_out` (wgs * 256 cells) and
// `inject` (n_inject rows of 5 int64) may be null.
inline void launch_cu_valu_signature(hipStream_t stream, void* report,
                                     void* where, int64_t wgs, uint64_t seed,
                                     int rounds, const void* expected,
                                     void* sig_out, const void* inject,
                                     int n_inject) {
  hipLaunchKernelGGL(cu_valu_signature_kernel, dim3((uint32_t)wgs),
                     dim3(kCuWgThreads), 0, stream,
                     static_cast<unsigned long long*>(report),
                     static_cast<int*>(where), seed, rounds,
                     static_cast<const u4*>(expected),
                     static_cast<u4*>(sig_out),
                     static_cast<const long long*>(inject), n_inject);
}

}  // namespace k3samd_kern
