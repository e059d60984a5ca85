// Pieces the GPU payload programs (mi-stream, mi-mxgemm, mi-cutest,
// mi-hostlink) share: the HIP error macro, the command-line flag matcher,
// the device opener, an owning device buffer, event timing, sysfs thermal
// sampling, and the host side of the memtest / gemmtest report with its
// detector drill and the drill's verdict lines. The verified-GEMM driver of
// mi-stream --gemmtest and mi-mxgemm builds on these in gemm_verify.h. Each
// payload is one translation unit, so everything here sits in an unnamed
// namespace.
//
// Define K3_PAYLOAD_NAME (the program's name as a string literal, the prefix
// of its error messages) before including this header.

#pragma once

#ifndef K3_PAYLOAD_NAME
#error "define K3_PAYLOAD_NAME before including payload_common.h"
#endif

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>

#include "../../k3samd/ops/hip/memtest_kernels.h"
#include "../topology/gpu_health.h"
#include "../topology/kfd_topology.h"

#define HIP_CHECK(x)                                                         \
  do {                                                                       \
    hipError_t err_ = (x);                                                   \
    if (err_ != hipSuccess) {                                                \
      std::fprintf(stderr, K3_PAYLOAD_NAME ": %s failed: %s\n", #x,          \
                   hipGetErrorString(err_));                                 \
      return 1;                                                              \
    }                                                                        \
  } while (0)

namespace {

// ---- command line ----

constexpr int kRun = -1;  // parse_options: no exit status yet, go on

// flag(name, n): argv[i] is `name` and n more arguments follow it, so a flag
// short of its values matches nothing and falls through to the usage text.
struct FlagMatcher {
  int argc;
  char** argv;
  int i;
  bool operator()(const char* name, int n_values = 0) const {
    return !std::strcmp(argv[i], name) && i + n_values < argc;
  }
};

// What no flag matched: print the usage text; --help is status 0, else 2.
int usage_status(const char* usage, const char* arg) {
  std::printf("%s", usage);
  return !std::strcmp(arg, "--help") ? 0 : 2;
}

// ---- device ----

// Count the visible GPUs into *ndev (none is an error). With `prop`, also
// select `device` and read its properties, an empty name (some boxes report
// none) replaced by "AMD GPU"; without, no device is selected.
int open_device(int device, int* ndev, hipDeviceProp_t* prop) {
  HIP_CHECK(hipGetDeviceCount(ndev));
  if (*ndev == 0) {
    std::fprintf(stderr, K3_PAYLOAD_NAME ": no GPUs visible\n");
    return 1;
  }
  if (!prop) return 0;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipGetDeviceProperties(prop, device));
  if (!prop->name[0]) std::strcpy(prop->name, "AMD GPU");
  return 0;
}

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t) {
  return std::chrono::duration<double>(Clock::now() - t).count();
}

// Owning device allocation: move-only (the move constructor deletes the
// copies), freed by the destructor, so every early return releases it.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  ~DevBuf() { (void)hipFree(p_); }  // hipFree(nullptr) is a no-op
  hipError_t alloc(size_t bytes) { return hipMalloc((void**)&p_, bytes); }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// "Warm up, then best of N between two events" on the null stream: `warm`
// untimed calls of launch(true) and a device sync, then the smallest time
// of `reps` calls of launch(false). The counts decide what a printed rate
// means, so each call site states its own.
struct EventTimer {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // created on first use

  template <typename Launch>
  int best_of(int warm, int reps, Launch&& launch, float* best_ms) {
    if (!ev0) {
      HIP_CHECK(hipEventCreate(&ev0));
      HIP_CHECK(hipEventCreate(&ev1));
    }
    for (int w = 0; w < warm; ++w) launch(true);
    HIP_CHECK(hipDeviceSynchronize());
    *best_ms = 1e30f;
    for (int rep = 0; rep < reps; ++rep) {
      float ms;
      HIP_CHECK(hipEventRecord(ev0));
      launch(false);
      HIP_CHECK(hipEventRecord(ev1));
      HIP_CHECK(hipEventSynchronize(ev1));
      HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
      if (ms < *best_ms) *best_ms = ms;
    }
    HIP_CHECK(hipGetLastError());
    return 0;
  }
};

// Best-effort temperature/power sampling of the first GPU from sysfs; a
// field the box does not expose reads -1.
struct ThermalSampler {
  int card = -1;
  long max_temp_c = -1;
  double max_power_w = -1.0;
  char cells[32] = "";  // "temp power" of the last sample, for a status line

  ThermalSampler() {
    auto topo = k3samd::enumerate_topology(k3samd::default_sysfs_root());
    if (!topo.gpus.empty()) card = topo.gpus[0].card_index;
  }
  k3samd::GpuRuntimeStats sample() {
    auto st = k3samd::read_runtime_stats(k3samd::default_sysfs_root(), card);
    const long temp_c = st.temp_mc < 0 ? -1 : st.temp_mc / 1000;
    const double power_w = st.power_uw < 0 ? -1.0 : st.power_uw / 1e6;
    if (temp_c > max_temp_c) max_temp_c = temp_c;
    if (power_w > max_power_w) max_power_w = power_w;
    std::snprintf(cells, sizeof(cells), "%5ldC %6.0fW", temp_c, power_w);
    return st;
  }
};

// Host copy of the device report that mem_verify*/buf_compare accumulate.
struct HostMemReport {
  long long v[k3samd_kern::kMemReportLen];
  long long bad_dwords() const { return v[0]; }
  long long bad_bits() const { return v[1]; }
  unsigned long long first() const { return (unsigned long long)v[2]; }
  unsigned xor_or() const { return (unsigned)v[3]; }
  int n_log() const {
    return (int)std::min<long long>(v[4], k3samd_kern::kMemLogSlots);
  }
  // log record i: {dword or element index, expected, actual}
  const long long* log(int i) const {
    return v + k3samd_kern::kMemReportHeader + 3 * i;
  }
};

int mem_report_reset(void* d_report) {
  HostMemReport r{};
  r.v[2] = -1;  // all-ones: identity of the unsigned min
  HIP_CHECK(hipMemcpy(d_report, r.v, sizeof(r.v), hipMemcpyHostToDevice));
  return 0;
}

// XOR `mask` into dword `g` of the buffer with two 4-byte copies.
int mem_flip(void* buf, uint64_t g, uint32_t mask) {
  uint32_t w;
  char* p = static_cast<char*>(buf) + g * 4;
  HIP_CHECK(hipMemcpy(&w, p, 4, hipMemcpyDeviceToHost));
  w ^= mask;
  HIP_CHECK(hipMemcpy(p, &w, 4, hipMemcpyHostToDevice));
  return 0;
}

// Detector drill of the memtest, gemmtest, mxgemmtest and cutest self-tests: a
// detector that has never fired proves nothing, so each flips three known
// bits and requires exactly those three back, by count, first index,
// xor-or and log. `index` ascends; `expect` is the dword before the flip.
struct DrillFlip {
  uint64_t index;
  uint32_t expect, mask;
};

bool drill_passed(const HostMemReport& r, const DrillFlip (&flips)[3],
                  int* caught) {
  *caught = 0;
  for (const DrillFlip& f : flips)
    for (int s = 0; s < r.n_log(); ++s) {
      const long long* rec = r.log(s);
      if ((uint64_t)rec[0] == f.index && (uint32_t)rec[1] == f.expect &&
          (uint32_t)rec[2] == (f.expect ^ f.mask)) {
        ++*caught;
        break;
      }
    }
  return *caught == 3 && r.bad_dwords() == 3 && r.bad_bits() == 3 &&
         r.first() == flips[0].index && r.v[4] == 3 &&
         r.xor_or() == (flips[0].mask | flips[1].mask | flips[2].mask);
}

// The tail every drill shares. `words` are the program's tag, the drill's
// name with a trailing space (or ""), the unit of the report's count and the
// success sentence: "<tag> selftest: FAIL (<drill>caught c/3, <unit> ...)"
// and status 3, or "<tag> selftest: <ok>" and 0.
struct DrillWords {
  const char *tag, *drill, *unit, *ok;
};

int drill_verdict(const HostMemReport& r, const DrillFlip (&flips)[3],
                  const DrillWords& w) {
  int caught;
  if (!drill_passed(r, flips, &caught)) {
    std::printf("%s selftest: FAIL (%scaught %d/3, %s %lld, bad_bits %lld, "
                "xor_or 0x%08x)\n",
                w.tag, w.drill, caught, w.unit, r.bad_dwords(), r.bad_bits(),
                r.xor_or());
    return 3;
  }
  std::printf("%s selftest: %s\n", w.tag, w.ok);
  return 0;
}

int mem_report_download(HostMemReport& r, const void* d_report) {
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  return 0;
}

// The same on a device report, downloaded first (1 on a HIP error).
int drill_verdict(const void* d_report, const DrillFlip (&flips)[3],
                  const DrillWords& w) {
  HostMemReport r;
  if (mem_report_download(r, d_report)) return 1;
  return drill_verdict(r, flips, w);
}

}  // namespace
