// Host-link (PCIe) test, host side: the pointer-chase table, its expected
// result, and a threaded fill / verify of the memtest pattern in host
// memory. No HIP include, so a plain host compiler can use it; numpy
// reproduces it in k3samd/ops/hostlink.py.
//
// Chase table: n slots of 64 bytes (one slot per cache line, so no hop is
// served by the line the previous one brought in), n a power of two,
// 2 <= n <= 2^26. Dword 0 of slot i holds
//   next(i) = (0x9E3779B1 * i + (lo32(seed) | 1)) & (n - 1)
// a full-period LCG mod n (multiplier = 1 mod 4, odd increment: Hull-Dobell),
// so a walk from slot 0 visits every slot once per n hops. The other 15
// dwords of a slot are zero. A walk of `hops` dependent loads yields
// (final, xor): the last loaded index and the XOR of every loaded index.
//
// host_verify fills the report layout of memtest_kernels.h (long long[56]:
// bad_dwords, bad_bits, first_bad_dword, xor_or, log_claims, 3 reserved,
// then up to 16 records of (g, expected, actual)) and accumulates like the
// device kernels do. Its answer does not depend on the thread count: each
// worker owns one contiguous range and the logs are merged in range order,
// so the log holds the 16 lowest bad dwords.

#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "memtest_pattern.h"

namespace k3samd_kern {

constexpr int kLinkSlotBytes = 64;
constexpr int kLinkSlotDwords = kLinkSlotBytes / 4;
constexpr int64_t kLinkChaseMaxN = 1ll << 26;
constexpr int64_t kLinkChaseMaxHops = 1ll << 22;  // seconds, not minutes
constexpr uint32_t kLinkChaseMul = 0x9E3779B1u;
constexpr int kLinkMaxHostThreads = 16;
constexpr int kLinkReportLen = 56;  // == kMemReportLen (memtest_kernels.h)
constexpr int kLinkLogSlots = 16;   // == kMemLogSlots

K3_MEMTEST_HD inline bool link_chase_n_ok(int64_t n) {
  return n >= 2 && n <= kLinkChaseMaxN && (n & (n - 1)) == 0;
}

K3_MEMTEST_HD inline uint32_t link_chase_next(uint32_t i, uint64_t seed,
                                              uint32_t n) {
  return (kLinkChaseMul * i + ((uint32_t)seed | 1u)) & (n - 1u);
}

struct LinkChaseResult {
  uint32_t final_index, xor_all;
};

// What `hops` dependent loads from slot 0 of a clean table return.
inline LinkChaseResult link_chase_expected(uint32_t n, uint64_t seed,
                                           uint64_t hops) {
  LinkChaseResult r{0u, 0u};
  for (uint64_t h = 0; h < hops; ++h) {
    r.final_index = link_chase_next(r.final_index, seed, n);
    r.xor_all ^= r.final_index;
  }
  return r;
}

inline void link_chase_fill(void* buf, uint32_t n, uint64_t seed) {
  uint32_t* p = static_cast<uint32_t*>(buf);
  std::memset(p, 0, (size_t)n * kLinkSlotBytes);
  for (uint32_t i = 0; i < n; ++i)
    p[(size_t)i * kLinkSlotDwords] = link_chase_next(i, seed, n);
}

// Worker count for a region: `requested` (> 0) or the machine's
// concurrency, never more than 16 and never more than one per 64 Ki cells.
inline int link_host_threads(int64_t n_cells, int requested) {
  int t = requested > 0 ? requested
                        : (int)std::max(1u, std::thread::hardware_concurrency());
  t = std::min(t, kLinkMaxHostThreads);
  const int64_t by_size = n_cells / 65536 + 1;
  if (requested <= 0 && by_size < t) t = (int)by_size;
  return (int)std::max<int64_t>(1, std::min<int64_t>(t, n_cells));
}

// Run fn(t, begin, end) over [0, n_cells) split into `threads` contiguous
// ranges, t = 0 .. threads - 1; the calling thread takes range 0.
template <typename Fn>
inline void link_host_parallel(int64_t n_cells, int threads, Fn fn) {
  std::vector<std::thread> pool;
  const int64_t per = (n_cells + threads - 1) / threads;
  for (int t = 1; t < threads; ++t) {
    const int64_t b = std::min(n_cells, per * t);
    const int64_t e = std::min(n_cells, b + per);
    pool.emplace_back(fn, t, b, e);
  }
  fn(0, (int64_t)0, std::min(n_cells, per));
  for (std::thread& th : pool) th.join();
}

inline void host_fill(void* buf, int64_t n_cells, MemSpec spec,
                      uint64_t cell_offset, int threads = 0) {
  if (n_cells <= 0) return;
  MemCell* p = static_cast<MemCell*>(buf);
  link_host_parallel(n_cells, link_host_threads(n_cells, threads),
                     [=](int, int64_t b, int64_t e) {
                       for (int64_t i = b; i < e; ++i)
                         p[i] = memtest_cell(spec, cell_offset + (uint64_t)i);
                     });
}

inline void host_report_reset(long long* report) {
  std::memset(report, 0, sizeof(long long) * kLinkReportLen);
  report[2] = -1;  // all-ones: identity of the unsigned min
}

// Compare [buf, buf + 16 * n_cells) with the pattern and accumulate into
// `report` (see the head of this file).
inline void host_verify(const void* buf, int64_t n_cells, MemSpec spec,
                        uint64_t cell_offset, long long* report,
                        int threads = 0) {
  if (n_cells <= 0) return;
  struct Part {
    unsigned long long bad = 0, bits = 0, first = ~0ull;
    uint32_t x_or = 0;
    int n_log = 0;
    unsigned long long log[kLinkLogSlots][3];
  };
  const int nt = link_host_threads(n_cells, threads);
  std::vector<Part> parts((size_t)nt);
  const MemCell* p = static_cast<const MemCell*>(buf);
  Part* out = parts.data();
  link_host_parallel(n_cells, nt, [=](int t, int64_t b, int64_t e) {
    Part part;
    for (int64_t i = b; i < e; ++i) {
      const uint64_t c = cell_offset + (uint64_t)i;
      const MemCell want = memtest_cell(spec, c);
      if (!std::memcmp(&want, &p[i], sizeof(MemCell))) continue;
      for (int k = 0; k < 4; ++k) {
        const uint32_t diff = want.d[k] ^ p[i].d[k];
        if (!diff) continue;
        const unsigned long long g = 4ull * c + (unsigned)k;
        ++part.bad;
        part.bits += (unsigned)__builtin_popcount(diff);
        part.x_or |= diff;
        if (g < part.first) part.first = g;
        if (part.n_log < kLinkLogSlots) {
          part.log[part.n_log][0] = g;
          part.log[part.n_log][1] = want.d[k];
          part.log[part.n_log][2] = p[i].d[k];
          ++part.n_log;
        }
      }
    }
    out[t] = part;
  });
  for (const Part& part : parts) {
    report[0] += (long long)part.bad;
    report[1] += (long long)part.bits;
    if (part.first < (unsigned long long)report[2])
      report[2] = (long long)part.first;
    report[3] |= (long long)part.x_or;
    for (int s = 0; s < part.n_log && report[4] < kLinkLogSlots; ++s) {
      long long* rec = report + 8 + 3 * report[4]++;
      for (int j = 0; j < 3; ++j) rec[j] = (long long)part.log[s][j];
    }
  }
}

}  // namespace k3samd_kern
