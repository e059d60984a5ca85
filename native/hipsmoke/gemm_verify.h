// The verified-GEMM driver of `mi-stream --gemmtest` and `mi-mxgemm`: fill
// the operands, compute the gold once without the matrix pipes, then loop
// MFMA GEMM -> bitwise compare, attributing every bad element to the XCC /
// HW_ID of the workgroup that produced it. Include after payload_common.h;
// like that file, everything sits in an unnamed namespace.
//
// The driver is a template over a *problem* type that supplies only what
// differs between the operand formats:
//
//   using Result;                        element of C and of the gold: float,
//                                        int32_t or double
//   static constexpr int kPoison;        the byte C is preset with, so that
//                                        an element the kernel skipped cannot
//                                        equal the gold: 0xFF (NaN) for float
//                                        and double; 0x80 for int32, where -1
//                                        is a legitimate product and
//                                        0x80808080 lies outside +-2^23
//   static constexpr const char* kTag;   "gemmtest" / "mxgemmtest"
//   static constexpr int64_t kSelftestK; K of the 256 x 256 self-test product
//   P fresh() const;                     an unallocated problem of the same
//                                        format, for the self-test
//   int alloc(m, n, k);                  operand (and scale) buffers; 0 or 1
//   void fill(seed);                     the launch_* calls, on the null
//   void gemm(c, where);                 stream
//   void ref(gold);
//   Result host_elem(seed, row, col);    exact host value of one element,
//                                        straight from the generator
//   std::vector<Result> host_product(seed);  the whole host product, operand
//                                        tables built once
//   void print_product_verdict(bad_mfma, bad_gold);  the self-test's lines
//                                        about the product, FAIL line included
//   const char* label();                 what precedes MxNxK in the header
//                                        line: "" or "fp8 "
//
// gemm_verify() returns 0 when the loop ran to its end, clean or not, with
// the figures in GemmVerifyResult (the caller prints its own JSON line and
// turns a miscompare into exit status 4); 1 on a HIP error; 3 when the
// self-test or the gold spot-check failed.
//
// The compare reports 32-bit dwords. With a 4-byte Result a dword index is
// the element index row * N + col; with double it is 2 * element + half
// (half 0 = the low dword), and a miscompare line ends in " half 0|1".

#pragma once

#include <cstring>
#include <vector>

#include "../../k3samd/ops/hip/gemm_kernels.h"

namespace {

struct GemmVerifyResult {
  long long iters = 0;
  double total_s = 0;
  float gold_ms = 0;
  HostMemReport report{};
  // of the lowest bad element; -1 when clean
  long long first_bad_row = -1, first_bad_col = -1;
  int first_bad_xcc = -1;
  long max_temp_c = -1;
  double max_power_w = -1.0;
  bool clean() const { return report.bad_dwords() == 0; }
  // average rate of the whole loop, compares and host syncs included
  double tflops(int64_t m, int64_t n, int64_t k) const {
    return iters * (2.0 * (double)m * (double)n * (double)k) / total_s / 1e12;
  }
};

// C and gold of an M x N problem and the per-tile XCC_ID/HW_ID record.
template <typename Result>
struct GemmResultBufs {
  DevBuf<Result> c, gold;
  DevBuf<int> where;
  int64_t tiles = 0;

  int alloc(int64_t m, int64_t n, int poison) {
    const size_t bytes = (size_t)m * n * sizeof(Result);
    tiles = (m / k3samd_kern::kGemmBM) * (n / k3samd_kern::kGemmBN);
    HIP_CHECK(c.alloc(bytes));
    HIP_CHECK(gold.alloc(bytes));
    HIP_CHECK(where.alloc((size_t)tiles * 8));
    HIP_CHECK(hipMemset(c, poison, bytes));  // unwritten != gold
    HIP_CHECK(hipMemset(where, 0xFF, (size_t)tiles * 8));
    return 0;
  }
};

// Self-test: (1) a 256 x 256 x kSelftestK product, the MFMA result and the
// integer gold, each against the host product of the generator; (2) the
// detector drill on C against the gold.
// Returns 0 ok, 3 failed, 1 HIP error.
template <typename Problem>
int gemm_verify_selftest(Problem p, void* d_report) {
  const int64_t m = 256, n = 256, k = Problem::kSelftestK;
  const uint64_t seed = 0x5EEDF00Dull;
  using Result = typename Problem::Result;
  constexpr size_t kBytes = sizeof(Result);
  constexpr uint64_t kDwords = kBytes / 4;  // report dwords per element
  GemmResultBufs<Result> g;
  if (p.alloc(m, n, k) || g.alloc(m, n, Problem::kPoison)) return 1;
  p.fill(seed);
  p.ref(g.gold);
  p.gemm(g.c, g.where);
  HIP_CHECK(hipGetLastError());
  std::vector<Result> hc(m * n), hg(m * n);
  HIP_CHECK(hipMemcpy(hc.data(), g.c, hc.size() * kBytes,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hg.data(), g.gold, hg.size() * kBytes,
                      hipMemcpyDeviceToHost));
  const std::vector<Result> want = p.host_product(seed);
  // bitwise (stricter than !=), as the main loop compares C with the gold
  long long bad_mfma = 0, bad_gold = 0;
  for (int64_t e = 0; e < m * n; ++e) {
    if (std::memcmp(&hc[e], &want[e], kBytes)) ++bad_mfma;
    if (std::memcmp(&hg[e], &want[e], kBytes)) ++bad_gold;
  }
  p.print_product_verdict(bad_mfma, bad_gold);
  if (bad_mfma || bad_gold) return 3;

  DrillFlip flips[3] = {{0, 0, 1u << 0},
                        {12345, 0, 1u << 17},
                        {(uint64_t)(m * n) * kDwords - 1, 0, 1u << 31}};
  for (DrillFlip& f : flips) {
    std::memcpy(&f.expect, (const char*)hg.data() + f.index * 4, 4);
    if (mem_flip(g.c, f.index, f.mask)) return 1;
  }
  if (mem_report_reset(d_report)) return 1;
  k3samd_kern::launch_buf_compare(0, g.c, g.gold, m * n * kBytes / 16,
                                  d_report);
  HIP_CHECK(hipGetLastError());
  return drill_verdict(d_report, flips,
                       {Problem::kTag, "", "bad_elems",
                        "detector caught 3/3 injected flips"});
}

// Exactly one of `iters` / `seconds` is positive; `inject` single-bit flips
// go into the first result before its compare.
template <typename Problem>
int gemm_verify(Problem& p, int64_t m, int64_t n, int64_t k, int iters,
                int seconds, int inject, bool selftest, GemmVerifyResult* out) {
  using namespace k3samd_kern;
  const char* const tag = Problem::kTag;
  const uint64_t seed = 0;
  using Result = typename Problem::Result;
  constexpr size_t kBytes = sizeof(Result);
  constexpr uint64_t kDwords = kBytes / 4;  // report dwords per element
  DevBuf<long long> d_report;
  HIP_CHECK(d_report.alloc(sizeof(long long) * kMemReportLen));
  if (selftest) {
    int rc = gemm_verify_selftest(p.fresh(), d_report);
    if (rc) return rc;
  }
  GemmResultBufs<Result> g;
  if (p.alloc(m, n, k) || g.alloc(m, n, Problem::kPoison)) return 1;
  p.fill(seed);
  // one timed launch, no warm-up
  if (EventTimer().best_of(0, 1, [&](bool) { p.ref(g.gold); }, &out->gold_ms))
    return 1;

  // gold spot-check: 64 fixed elements against host integer dot products
  // of the generator — independent of the device entirely
  for (int i = 0; i < 64; ++i) {
    const uint32_t row = i == 63 ? (uint32_t)(m - 1)
                                 : (uint32_t)(((uint64_t)i * 0x9E3779B1ull) % (uint64_t)m);
    const uint32_t col = i == 63 ? (uint32_t)(n - 1)
                                 : (uint32_t)(((uint64_t)i * 0x85EBCA6Bull + 7) % (uint64_t)n);
    Result got;
    HIP_CHECK(hipMemcpy(&got, g.gold + (size_t)row * n + col, kBytes,
                        hipMemcpyDeviceToHost));
    const Result want = p.host_elem(seed, row, col);
    if (std::memcmp(&got, &want, kBytes)) {
      std::printf("%s: gold spot-check FAIL at [%u][%u]: device %.2f, "
                  "host %.2f\n", tag, row, col, (double)got, (double)want);
      return 3;
    }
  }
  std::printf("%s: %s%lldx%lldx%lld, gold by integer VALU in %.1f ms, "
              "spot-check 64/64 vs host%s\n",
              tag, p.label(), (long long)m, (long long)n, (long long)k,
              out->gold_ms, inject ? " [fault injection ON]" : "");

  ThermalSampler thermal;
  if (mem_report_reset(d_report)) return 1;
  const double flops_per = 2.0 * (double)m * (double)n * (double)k;
  std::printf("%6s %10s %12s %6s %7s\n", "t(s)", "iters", "TFLOP/s", "temp",
              "power");
  long long done = 0, done_last = 0;
  int batch = 1;
  const auto t0 = Clock::now();
  auto t_last = t0;
  double next_report = 2.0;
  auto status = [&] {
    thermal.sample();
    const double dt = seconds_since(t_last);
    std::printf("%6.0f %10lld %12.1f %s\n", seconds_since(t0), done,
                dt > 0 ? (done - done_last) * flops_per / dt / 1e12 : 0.0,
                thermal.cells);
    std::fflush(stdout);
    done_last = done;
    t_last = Clock::now();
  };
  while (seconds > 0 ? seconds_since(t0) < (double)seconds : done < iters) {
    int todo = batch;
    if (seconds <= 0 && todo > iters - done) todo = (int)(iters - done);
    const auto tb = Clock::now();
    for (int i = 0; i < todo; ++i) {
      p.gemm(g.c, g.where);
      if (done == 0 && i == 0 && inject > 0) {
        // operator alerting drill: N single-bit flips (bit f % 32) in the
        // first result before its compare, at elements evenly spaced from
        // 0 (of a double, in its low dword: half 0)
        const uint64_t step = (uint64_t)(m * n) / (uint64_t)inject;
        HIP_CHECK(hipDeviceSynchronize());
        for (int f = 0; f < inject; ++f)
          if (mem_flip(g.c, (uint64_t)f * step * kDwords, 1u << (f % 32)))
            return 1;
      }
      launch_buf_compare(0, g.c, g.gold, m * n * kBytes / 16, d_report);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    done += todo;
    // size the batch to ~0.2 s between host syncs
    const double per = seconds_since(tb) / todo;
    batch = per > 0 ? (int)(0.2 / per) : 64;
    if (batch < 1) batch = 1;
    if (batch > 64) batch = 64;
    if (seconds_since(t0) >= next_report) {
      status();
      next_report += 2.0;
    }
  }
  out->total_s = seconds_since(t0);
  if (done != done_last) status();  // the tail since the last line
  out->iters = done;
  out->max_temp_c = thermal.max_temp_c;
  out->max_power_w = thermal.max_power_w;

  const HostMemReport& r = out->report;
  if (mem_report_download(out->report, d_report)) return 1;
  std::vector<int> where((size_t)g.tiles * 2);
  HIP_CHECK(hipMemcpy(where.data(), g.where, where.size() * 4,
                      hipMemcpyDeviceToHost));
  auto xcc_of = [&](unsigned long long dword, unsigned* hw_id) {
    const unsigned long long elem = dword / kDwords;
    const int64_t row = (int64_t)(elem / (uint64_t)n), col = (int64_t)(elem % (uint64_t)n);
    const int64_t tile = (row / kGemmBM) * (n / kGemmBN) + col / kGemmBN;
    if (hw_id) *hw_id = (unsigned)where[2 * tile + 1];
    return where[2 * tile] & 0xF;
  };
  if (!out->clean()) {
    out->first_bad_row = (long long)(r.first() / kDwords / (uint64_t)n);
    out->first_bad_col = (long long)(r.first() / kDwords % (uint64_t)n);
    out->first_bad_xcc = xcc_of(r.first(), nullptr);
    std::printf("%s: MISCOMPARE - %lld element(s), %lld bit(s)\n", tag,
                r.bad_dwords(), r.bad_bits());
    for (int i = 0; i < r.n_log(); ++i) {
      const long long* rec = r.log(i);
      unsigned hw_id = 0;
      const int xcc = xcc_of((unsigned long long)rec[0], &hw_id);
      const unsigned long long elem = (unsigned long long)rec[0] / kDwords;
      std::printf("C[%llu][%llu] expected 0x%08x actual 0x%08x xor 0x%08x "
                  "xcc %d hw_id 0x%08x",
                  elem / (unsigned long long)n, elem % (unsigned long long)n,
                  (unsigned)rec[1], (unsigned)rec[2],
                  (unsigned)(rec[1] ^ rec[2]), xcc, hw_id);
      if constexpr (kDwords == 2)
        std::printf(" half %d", (int)((unsigned long long)rec[0] & 1));
      std::printf("\n");
    }
  }
  return 0;
}

}  // namespace
