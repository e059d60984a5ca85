// HBM pattern memory-test kernels (gfx950), shared by the torch extension
// (k3samd_kernels.hip) and the standalone payload
// (native/hipsmoke/mi_stream.hip) the same way stream_kernels.h is.
// Pure HIP, plain C++ and builtins only.
//
// Shape: the STREAM suite's — one 16-byte vector access per lane, 256
// threads per block, flat grid, launch_chunked for regions >= 64 GiB (the
// chunk's cell offset is passed into the kernel so the pattern stays a
// function of the absolute cell index).
//
// Report (device-resident int64[kMemReportLen], accumulated across calls):
//   [0] bad_dwords       count of mismatching dwords
//   [1] bad_bits         popcount of all XOR differences
//   [2] first_bad_dword  unsigned min of mismatching global dword indices,
//                        initialised to all-ones (reads as -1 = none)
//   [3] xor_or           OR of all 32-bit XOR differences
//   [4] log_claims       log slots claimed (may run a little past 16)
//   [5..7] reserved, zero
//   [8..] up to 16 records (g, expected, actual), first come first served
//
// Cost model: a clean pass issues ZERO atomics — the mismatch flag is
// reduced across the wave with one __ballot, and everything else happens
// only in waves that saw a mismatch (one lane per wave then issues the
// 64-bit add/min/or). Log slots are claimed with an atomic only after a
// plain load of the claim counter reads < 16, so a fully corrupted buffer
// does not serialise one atomic per dword on a single address.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "memtest_pattern.h"
#include "stream_kernels.h"

namespace k3samd_kern {

constexpr int kMemLogSlots = 16;
constexpr int kMemReportHeader = 8;
constexpr int kMemReportLen = kMemReportHeader + 3 * kMemLogSlots;

using u4 = __attribute__((ext_vector_type(4))) unsigned int;

__device__ __forceinline__ u4 mem_expected(const MemSpec& spec, uint64_t c) {
  MemCell e = memtest_cell(spec, c);
  u4 v = {e.d[0], e.d[1], e.d[2], e.d[3]};
  return v;
}

// Fold one lane's XOR difference into the report. EVERY lane of the wave
// must call this (lanes past the end pass diff = 0): it contains cross-lane
// operations. `c` is the lane's absolute cell index.
__device__ __forceinline__ void mem_account(unsigned long long* report,
                                            uint64_t c, u4 expect, u4 diff) {
  const bool lane_bad = (diff.x | diff.y | diff.z | diff.w) != 0u;
  if (__ballot(lane_bad) == 0ull) return;  // wave-uniform: clean wave, done

  unsigned long long n_bad = 0, n_bits = 0, x_or = 0;
  unsigned long long first = ~0ull;
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    if (diff[k] != 0u) {
      ++n_bad;
      n_bits += (unsigned)__popc(diff[k]);
      x_or |= diff[k];
      first = 4ull * c + (unsigned)k;  // descending k: ends at the smallest
    }
  }
  // counts fit in 32 bits per wave (<= 64*4 dwords, <= 64*128 bits)
  unsigned bad32 = (unsigned)n_bad, bits32 = (unsigned)n_bits;
  unsigned or32 = (unsigned)x_or;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    bad32 += __shfl_xor(bad32, m, 64);
    bits32 += __shfl_xor(bits32, m, 64);
    or32 |= __shfl_xor(or32, m, 64);
    unsigned long long o = __shfl_xor(first, m, 64);
    first = o < first ? o : first;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&report[0], (unsigned long long)bad32);
    atomicAdd(&report[1], (unsigned long long)bits32);
    atomicMin(&report[2], first);
    atomicOr(&report[3], (unsigned long long)or32);
  }
  if (lane_bad) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (diff[k] == 0u) continue;
      // plain (non-RMW) load first: once the log is full nobody queues
      // on the claim counter any more
      unsigned long long seen = __hip_atomic_load(
          &report[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (seen >= (unsigned long long)kMemLogSlots) break;
      unsigned long long slot = atomicAdd(&report[4], 1ull);
      if (slot >= (unsigned long long)kMemLogSlots) break;
      unsigned long long* rec = report + kMemReportHeader + 3 * slot;
      rec[0] = 4ull * c + (unsigned)k;
      rec[1] = expect[k];
      rec[2] = expect[k] ^ diff[k];  // what memory actually held
    }
  }
}

template <bool NT>
__global__ void mem_fill_kernel(u4* __restrict__ p, int64_t n_cells,
                                uint64_t cell_offset, MemSpec spec) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;  // no cross-lane operation in this kernel
  u4 v = mem_expected(spec, cell_offset + (uint64_t)i);
  if constexpr (NT) {
    __builtin_nontemporal_store(v, &p[i]);
  } else {
    p[i] = v;
  }
}

// Streaming read with zero reuse: the load is non-temporal like the NT
// STREAM kernels' loads.
__global__ void mem_verify_kernel(const u4* __restrict__ p, int64_t n_cells,
                                  uint64_t cell_offset, MemSpec spec,
                                  unsigned long long* __restrict__ report) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < n_cells;
  const uint64_t c = cell_offset + (uint64_t)i;
  u4 expect = mem_expected(spec, c);
  u4 diff = {0u, 0u, 0u, 0u};
  if (in_range) diff = __builtin_nontemporal_load(&p[i]) ^ expect;
  mem_account(report, c, expect, diff);  // all lanes, no early return
}

// Moving-inversions march element: verify `old_spec`, write `new_spec` to
// the same cell — one read and one write per cell.
template <bool NT>
__global__ void mem_verify_fill_kernel(u4* __restrict__ p, int64_t n_cells,
                                       uint64_t cell_offset, MemSpec old_spec,
                                       MemSpec new_spec,
                                       unsigned long long* __restrict__ report) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_range = i < n_cells;
  const uint64_t c = cell_offset + (uint64_t)i;
  u4 expect = mem_expected(old_spec, c);
  u4 diff = {0u, 0u, 0u, 0u};
  if (in_range) {
    u4 next = mem_expected(new_spec, c);
    if constexpr (NT) {
      diff = __builtin_nontemporal_load(&p[i]) ^ expect;
      __builtin_nontemporal_store(next, &p[i]);
    } else {
      diff = p[i] ^ expect;
      p[i] = next;
    }
  }
  mem_account(report, c, expect, diff);
}

// ---- host-side launchers (chunked; no sync, errors via hipGetLastError) ----

inline void launch_mem_fill(hipStream_t stream, void* buf, int64_t n_cells,
                            uint64_t cell_offset, MemSpec spec, bool nt) {
  u4* p = static_cast<u4*>(buf);
  launch_chunked(n_cells, [&](int64_t off, int64_t cnt) {
    dim3 g((uint32_t)stream_grid(cnt)), b(kThreadsPerBlock);
    if (nt) {
      hipLaunchKernelGGL(mem_fill_kernel<true>, g, b, 0, stream, p + off, cnt,
                         cell_offset + (uint64_t)off, spec);
    } else {
      hipLaunchKernelGGL(mem_fill_kernel<false>, g, b, 0, stream, p + off,
                         cnt, cell_offset + (uint64_t)off, spec);
    }
  });
}

inline void launch_mem_verify(hipStream_t stream, const void* buf,
                              int64_t n_cells, uint64_t cell_offset,
                              MemSpec spec, void* report) {
  const u4* p = static_cast<const u4*>(buf);
  auto* r = static_cast<unsigned long long*>(report);
  launch_chunked(n_cells, [&](int64_t off, int64_t cnt) {
    dim3 g((uint32_t)stream_grid(cnt)), b(kThreadsPerBlock);
    hipLaunchKernelGGL(mem_verify_kernel, g, b, 0, stream, p + off, cnt,
                       cell_offset + (uint64_t)off, spec, r);
  });
}

inline void launch_mem_verify_fill(hipStream_t stream, void* buf,
                                   int64_t n_cells, uint64_t cell_offset,
                                   MemSpec old_spec, MemSpec new_spec,
                                   void* report, bool nt) {
  u4* p = static_cast<u4*>(buf);
  auto* r = static_cast<unsigned long long*>(report);
  launch_chunked(n_cells, [&](int64_t off, int64_t cnt) {
    dim3 g((uint32_t)stream_grid(cnt)), b(kThreadsPerBlock);
    if (nt) {
      hipLaunchKernelGGL(mem_verify_fill_kernel<true>, g, b, 0, stream,
                         p + off, cnt, cell_offset + (uint64_t)off, old_spec,
                         new_spec, r);
    } else {
      hipLaunchKernelGGL(mem_verify_fill_kernel<false>, g, b, 0, stream,
                         p + off, cnt, cell_offset + (uint64_t)off, old_spec,
                         new_spec, r);
    }
  });
}

}  // namespace k3samd_kern
