// Host-link (PCIe) test kernels (gfx950), shared by the torch extension
// (k3samd_kernels.hip) and the standalone payload
// (native/hipsmoke/mi_hostlink.hip). Pure HIP, plain C++ and builtins only,
// vector loads and stores only.
//
// Every `host` pointer is the device-visible address of coherent pinned
// host memory: each access crosses the link. The pattern, the report and
// the accounting are the memtest's (memtest_pattern.h, mem_expected,
// mem_account), so a miscompare found over the link reads like one found
// in HBM.
//
// Shape: unlike the flat HBM kernels the grid is capped and chosen by the
// caller (`wgs` workgroups of 256 lanes, 1..4096). The region is walked in
// tiles of kLinkUnroll * wgs * 256 cells; inside a tile a lane owns the
// cells  tile + u * wgs * 256 + wg * 256 + lane  (u < kLinkUnroll), so a
// wave's access is contiguous and a lane has kLinkUnroll independent
// 16-byte requests in flight before it compares the first. Bytes in flight
// on the link are  wgs * 256 * 16 * kLinkUnroll, a knob, not an accident of
// the buffer size. Whole tiles run unpredicated; the last, partial tile
// predicates each access, and every lane of every wave still reaches
// mem_account (it contains cross-lane operations): the trip counts depend
// on n_cells and the grid only.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hostlink_pattern.h"
#include "memtest_kernels.h"

namespace k3samd_kern {

static_assert(kLinkReportLen == kMemReportLen && kLinkLogSlots == kMemLogSlots,
              "hostlink_pattern.h restates the memtest report layout");

// Independent 16-byte requests per lane. The default is the measured choice
// (profiles/r08_hostlink.md); the macro exists for that sweep.
#ifndef K3_LINK_UNROLL
#define K3_LINK_UNROLL 4
#endif
constexpr int kLinkUnroll = K3_LINK_UNROLL;
static_assert(kLinkUnroll >= 1 && kLinkUnroll <= 16, "K3_LINK_UNROLL");
constexpr int kLinkMaxWgs = 4096;
constexpr int kLinkDefaultWgs = 256;  // per direction: one per CU
constexpr int kLinkThreads = 256;
constexpr int kLinkChaseOutLen = 4;  // final, xor, ticks, hops

__host__ __device__ inline bool link_wgs_ok(int64_t wgs) {
  return wgs >= 1 && wgs <= kLinkMaxWgs;
}

// Workgroup `wg` of `n_wgs` pull-verifies its share of the region.
__device__ __forceinline__ void link_pull_walk(
    const u4* __restrict__ host, int64_t n_cells, uint64_t cell_offset,
    const MemSpec& spec, unsigned long long* __restrict__ report, int64_t wg,
    int64_t n_wgs) {
  const int64_t stride = n_wgs * kLinkThreads;
  const int64_t tile = stride * kLinkUnroll;
  const int64_t lane0 = wg * kLinkThreads + threadIdx.x;
  int64_t base = 0;
  for (; base + tile <= n_cells; base += tile) {  // uniform over the grid
    u4 v[kLinkUnroll];
#pragma unroll
    for (int u = 0; u < kLinkUnroll; ++u)
      v[u] = __builtin_nontemporal_load(&host[base + u * stride + lane0]);
#pragma unroll
    for (int u = 0; u < kLinkUnroll; ++u) {
      const uint64_t c = cell_offset + (uint64_t)(base + u * stride + lane0);
      const u4 expect = mem_expected(spec, c);
      mem_account(report, c, expect, v[u] ^ expect);
    }
  }
  if (base < n_cells) {  // uniform: the partial tile, every lane enters
    u4 v[kLinkUnroll];
#pragma unroll
    for (int u = 0; u < kLinkUnroll; ++u) {
      const int64_t i = base + u * stride + lane0;
      v[u] = u4{0u, 0u, 0u, 0u};
      if (i < n_cells) v[u] = __builtin_nontemporal_load(&host[i]);
    }
#pragma unroll
    for (int u = 0; u < kLinkUnroll; ++u) {
      const int64_t i = base + u * stride + lane0;
      const uint64_t c = cell_offset + (uint64_t)i;
      const u4 expect = mem_expected(spec, c);
      u4 diff = {0u, 0u, 0u, 0u};
      if (i < n_cells) diff = v[u] ^ expect;
      mem_account(report, c, expect, diff);  // all lanes
    }
  }
}

// The same walk, storing the pattern (no cross-lane operation).
__device__ __forceinline__ void link_push_walk(u4* __restrict__ host,
                                               int64_t n_cells,
                                               uint64_t cell_offset,
                                               const MemSpec& spec, int64_t wg,
                                               int64_t n_wgs) {
  const int64_t stride = n_wgs * kLinkThreads;
  const int64_t tile = stride * kLinkUnroll;
  const int64_t lane0 = wg * kLinkThreads + threadIdx.x;
  for (int64_t base = 0; base < n_cells; base += tile) {
#pragma unroll
    for (int u = 0; u < kLinkUnroll; ++u) {
      const int64_t i = base + u * stride + lane0;
      if (i < n_cells)
        __builtin_nontemporal_store(
            mem_expected(spec, cell_offset + (uint64_t)i), &host[i]);
    }
  }
}

__global__ void __launch_bounds__(kLinkThreads)
link_pull_verify_kernel(const u4* __restrict__ host, int64_t n_cells,
                        uint64_t cell_offset, MemSpec spec,
                        unsigned long long* __restrict__ report) {
  link_pull_walk(host, n_cells, cell_offset, spec, report, blockIdx.x,
                 gridDim.x);
}

__global__ void __launch_bounds__(kLinkThreads)
link_push_fill_kernel(u4* __restrict__ host, int64_t n_cells,
                      uint64_t cell_offset, MemSpec spec) {
  link_push_walk(host, n_cells, cell_offset, spec, blockIdx.x, gridDim.x);
}

// One region of a duplex launch.
struct LinkRegion {
  void* host;
  int64_t n_cells;
  uint64_t cell_offset;
  MemSpec spec;
};

// Even workgroups pull-verify `pull`, odd workgroups push-fill `push`
// (disjoint regions): one wavefront population loads both directions of
// the link. The branch is uniform per workgroup. Needs a grid of >= 2.
__global__ void __launch_bounds__(kLinkThreads)
link_duplex_kernel(LinkRegion pull, LinkRegion push,
                   unsigned long long* __restrict__ report) {
  const int64_t wg = blockIdx.x >> 1;
  if ((blockIdx.x & 1u) == 0u) {
    link_pull_walk(static_cast<const u4*>(pull.host), pull.n_cells,
                   pull.cell_offset, pull.spec, report, wg,
                   (gridDim.x + 1) >> 1);
  } else {
    link_push_walk(static_cast<u4*>(push.host), push.n_cells,
                   push.cell_offset, push.spec, wg, gridDim.x >> 1);
  }
}

// Round-trip latency and dependent-load integrity: one lane walks the chase
// table of hostlink_pattern.h from slot 0 for `hops` loads. Each load is a
// system-scope atomic load (a vector load that no device cache serves), and
// each loaded index is masked with n - 1 before it is dereferenced: a
// corrupted slot changes the answer but never sends a load outside the
// table. out = {final, xor, wall_clock64 ticks, hops}.
__global__ void link_chase_kernel(const uint32_t* __restrict__ slots,
                                  uint32_t n, unsigned long long hops,
                                  unsigned long long* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t mask = n - 1u;
  uint32_t i = 0u, x = 0u;
  const unsigned long long t0 = wall_clock64();
  for (unsigned long long h = 0; h < hops; ++h) {
    i = __hip_atomic_load(&slots[(size_t)i * kLinkSlotDwords],
                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) &
        mask;
    x ^= i;
  }
  const unsigned long long t1 = wall_clock64();
  out[0] = i;
  out[1] = x;
  out[2] = t1 - t0;
  out[3] = hops;
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----
// Callers have checked: n_cells >= 1, link_wgs_ok(wgs) (duplex: wgs >= 2),
// link_chase_n_ok(n), 1 <= hops <= kLinkChaseMaxHops.

inline void launch_link_pull_verify(hipStream_t stream, const void* host,
                                    int64_t n_cells, uint64_t cell_offset,
                                    MemSpec spec, void* report, int wgs) {
  hipLaunchKernelGGL(link_pull_verify_kernel, dim3((uint32_t)wgs),
                     dim3(kLinkThreads), 0, stream,
                     static_cast<const u4*>(host), n_cells, cell_offset, spec,
                     static_cast<unsigned long long*>(report));
}

inline void launch_link_push_fill(hipStream_t stream, void* host,
                                  int64_t n_cells, uint64_t cell_offset,
                                  MemSpec spec, int wgs) {
  hipLaunchKernelGGL(link_push_fill_kernel, dim3((uint32_t)wgs),
                     dim3(kLinkThreads), 0, stream, static_cast<u4*>(host),
                     n_cells, cell_offset, spec);
}

inline void launch_link_duplex(hipStream_t stream, LinkRegion pull,
                               LinkRegion push, void* report, int wgs) {
  hipLaunchKernelGGL(link_duplex_kernel, dim3((uint32_t)wgs),
                     dim3(kLinkThreads), 0, stream, pull, push,
                     static_cast<unsigned long long*>(report));
}

inline void launch_link_chase(hipStream_t stream, const void* slots,
                              uint32_t n, uint64_t hops, void* out) {
  hipLaunchKernelGGL(link_chase_kernel, dim3(1), dim3(64), 0, stream,
                     static_cast<const uint32_t*>(slots), n,
                     (unsigned long long)hops,
                     static_cast<unsigned long long*>(out));
}

}  // namespace k3samd_kern
