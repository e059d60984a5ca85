// mi-stream — standalone CDNA4 STREAM + MFMA smoke payload for the
// validation pod.
//
// The MI355X-native replacement for the reference's in-pod `nvidia-smi`
// payload (/root/reference/nvidia-smi.yaml:13) with actual GPU work: an
// HBM3E STREAM suite (copy/scale/add/triad, plain + non-temporal) and an
// MFMA matrix-core warm-up that lights up all 8 XCDs, printing a
// golden-output-style table (the analog of README.md:137-156) plus one
// machine-readable JSON line. No torch dependency — links only the HIP
// runtime, so the smoke container stays small.
//
// Layout: the pieces the modes share, then one run_* function per mode;
// main() parses, validates and dispatches. The kernels and their launch_*
// helpers live in k3samd/ops/hip/*.h.
//
// Build: hipcc --offload-arch=gfx950 -O3 mi_stream.hip -o mi-stream

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../k3samd/ops/hip/gemm_dense_kernels.h"
#include "../../k3samd/ops/hip/gemm_kernels.h"
#include "../../k3samd/ops/hip/memtest_kernels.h"
#include "../../k3samd/ops/hip/stream_kernels.h"
#include "../topology/gpu_health.h"
#include "../topology/kfd_topology.h"

#define K3_PAYLOAD_NAME "mi-stream"
#include "payload_common.h"
#include "gemm_verify.h"

using k3samd_kern::f4;

namespace {

// ---- pieces the modes share (more of them in payload_common.h) ----

constexpr float kScalar = 2.5f;  // the s of scale and triad

double gbps(double bytes, float ms) { return bytes / (ms * 1e6); }
double tflops(double flops, float ms) { return flops / (ms * 1e9); }

constexpr int kNoGemmFormat = -1;

struct Options {
  int64_t mib = 1024;
  int iters = 20, device = 0;
  bool do_mfma = true, do_check = true;
  bool all_gpus = false, lds_compare = false, tune = false;
  int burn_s = 0;
  bool memtest = false;
  int passes = 1, vram_percent = 0, inject = 0;
  bool gemmtest = false;
  int64_t gemm_m = 4096, gemm_n = 4096, gemm_k = 4096;
  int gemm_iters = 0, gemm_seconds = 0, gemm_inject = 0;
  // --gemm-format: kNoGemmFormat without the flag, 0 = bf16, else a
  // k3samd_kern::kGemmFmt* id; the flag's word when it names no format
  int gemm_format = kNoGemmFormat;
  const char* gemm_format_bad = nullptr;
};

// Numerics self-check: the pod log doubles as a correctness oracle (the
// reference's nvidia-smi output carried version oracles the same way,
// /root/reference/README.md:139-147). Three checks against host-computed
// references: fp32 triad (exact), one bf16 MFMA tile, one block-scaled
// MX-fp8 tile (identity-A => must reproduce B exactly).
bool self_check() {
  using namespace k3samd_kern;
  // --- triad, 4096 elements, exactly-representable values
  {
    const int64_t n = 4096, n4 = n / 4;
    DevBuf<f4> a, b, c;
    (void)a.alloc(n * 4);
    (void)b.alloc(n * 4);
    (void)c.alloc(n * 4);
    std::vector<float> hb(n), hc(n), ha(n);
    for (int64_t i = 0; i < n; ++i) {
      hb[i] = (float)((i % 31) - 15);
      hc[i] = (float)((i % 17) - 8) * 0.5f;
    }
    (void)hipMemcpy(b, hb.data(), n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(c, hc.data(), n * 4, hipMemcpyHostToDevice);
    launch_stream_triad(0, a, b, c, kScalar, n4, true);
    (void)hipMemcpy(ha.data(), a, n * 4, hipMemcpyDeviceToHost);
    for (int64_t i = 0; i < n; ++i)
      if (ha[i] != hb[i] + kScalar * hc[i]) {
        std::printf("numerics: triad FAIL\n");
        return false;
      }
  }
  // --- bf16 MFMA tile vs host float reference
  double mfma_err = 0;
  {
    DevBuf<uint16_t> A, B;
    DevBuf<float> D;
    (void)A.alloc(16 * 32 * 2);
    (void)B.alloc(32 * 16 * 2);
    (void)D.alloc(16 * 16 * 4);
    std::vector<uint16_t> hA(16 * 32), hB(32 * 16);
    std::vector<float> fA(16 * 32), fB(32 * 16);
    auto to_bf16 = [](float f) -> uint16_t {
      uint32_t u;
      std::memcpy(&u, &f, 4);
      return (uint16_t)(u >> 16);  // values chosen exactly representable
    };
    for (int i = 0; i < 16 * 32; ++i) {
      fA[i] = (float)((i % 13) - 6) * 0.25f;
      hA[i] = to_bf16(fA[i]);
    }
    for (int i = 0; i < 32 * 16; ++i) {
      fB[i] = (float)((i % 11) - 5) * 0.5f;   // asymmetric vs A
      hB[i] = to_bf16(fB[i]);
    }
    (void)hipMemcpy(A, hA.data(), hA.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(B, hB.data(), hB.size() * 2, hipMemcpyHostToDevice);
    launch_mfma_gemm16(0, A, B, D, 0);
    std::vector<float> hD(256);
    (void)hipMemcpy(hD.data(), D, 256 * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        float ref = 0;
        for (int k = 0; k < 32; ++k) ref += fA[i * 32 + k] * fB[k * 16 + j];
        double e = std::abs(hD[i * 16 + j] - ref);
        if (e > mfma_err) mfma_err = e;
      }
    if (mfma_err > 1e-3) {
      std::printf("numerics: bf16 MFMA FAIL (err %g)\n", mfma_err);
      return false;
    }
  }
  // --- MX-fp8 identity tile: D must equal B rows exactly
  double mx_err = 0;
  {
    DevBuf<uint8_t> A, B;
    DevBuf<float> D;
    (void)A.alloc(16 * 128);
    (void)B.alloc(16 * 128);
    (void)D.alloc(16 * 16 * 4);
    std::vector<uint8_t> hA(16 * 128, 0), hB(16 * 128);
    for (int i = 0; i < 16; ++i) hA[i * 128 + i] = 0x38;  // e4m3 1.0 on diag
    // B values: exact small e4m3 codes, col-major pack, asymmetric
    std::vector<float> fB(128 * 16);
    const float lut[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    for (int k = 0; k < 128; ++k)
      for (int j = 0; j < 16; ++j) {
        int code = (k * 7 + j * 3) % 16;  // uses sign bit too
        float v = lut[code & 7] * ((code & 8) ? -1.f : 1.f);
        fB[k * 16 + j] = v;
        // e4m3 encodings of the lut: 0,0x30,0x38,0x3c,0x40,0x44,0x48,0x4c
        const uint8_t enc[8] = {0, 0x30, 0x38, 0x3c, 0x40, 0x44, 0x48, 0x4c};
        hB[j * 128 + k] = enc[code & 7] | ((code & 8) ? 0x80 : 0);
      }
    (void)hipMemcpy(A, hA.data(), hA.size(), hipMemcpyHostToDevice);
    (void)hipMemcpy(B, hB.data(), hB.size(), hipMemcpyHostToDevice);
    launch_mx_gemm16(0, 0, A, B, D);
    std::vector<float> hD(256);
    (void)hipMemcpy(hD.data(), D, 256 * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double e = std::abs(hD[i * 16 + j] - fB[i * 16 + j]);
        if (e > mx_err) mx_err = e;
      }
    if (mx_err != 0.0) {
      std::printf("numerics: MX-fp8 FAIL (err %g)\n", mx_err);
      return false;
    }
  }
  std::printf(
      "numerics: triad exact, bf16 MFMA err %.2g, MX-fp8 identity exact\n",
      mfma_err);
  return true;
}

// ---------------------------------------------------------------------------
// --memtest: HBM pattern memory test (kernels in memtest_kernels.h).
// Exit codes: 0 clean, 3 detector self-test failed, 4 data miscompare.
// ---------------------------------------------------------------------------

// Detector self-test: fill 1 MiB and run the detector drill on it.
// Returns 0 ok, 3 detector failed, 1 HIP error.
int mem_selftest(void* d_report) {
  using namespace k3samd_kern;
  const int64_t n_cells = (1 << 20) / 16;
  const MemSpec spec{0x5EEDF00Dull, kMemPatternAddr, 0};
  DevBuf<void> buf;
  HIP_CHECK(buf.alloc(n_cells * 16));
  launch_mem_fill(0, buf, n_cells, 0, spec, true);
  HIP_CHECK(hipDeviceSynchronize());
  DrillFlip flips[3] = {{0, 0, 1u << 0},
                        {4ull * 12345 + 2, 0, 1u << 17},
                        {4ull * n_cells - 1, 0, 1u << 31}};
  for (DrillFlip& f : flips) {
    f.expect = memtest_cell(spec, f.index / 4).d[f.index % 4];
    if (mem_flip(buf, f.index, f.mask)) return 1;
  }
  if (mem_report_reset(d_report)) return 1;
  launch_mem_verify(0, buf, n_cells, 0, spec, d_report);
  HIP_CHECK(hipGetLastError());
  return drill_verdict(d_report, flips,
                       {"memtest", "", "bad_dwords",
                        "detector caught 3/3 injected flips"});
}

// Host-side pattern dump (no HIP call): one cell per line, d0..d3 as hex.
int mem_pattern_dump(char** a) {
  const int pattern = std::atoi(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const bool invert = std::atoi(a[2]) != 0;
  const uint64_t off = std::strtoull(a[3], nullptr, 0);
  const uint64_t n = std::strtoull(a[4], nullptr, 0);
  if (pattern < 0 || pattern >= k3samd_kern::kMemPatternCount) {
    std::fprintf(stderr, "mi-stream: unknown memtest pattern %d\n", pattern);
    return 2;
  }
  for (uint64_t i = 0; i < n; ++i) {
    k3samd_kern::MemCell c =
        k3samd_kern::memtest_cell(pattern, seed, invert, off + i);
    std::printf("%08x %08x %08x %08x\n", c.d[0], c.d[1], c.d[2], c.d[3]);
  }
  return 0;
}

int run_memtest(const Options& o) {
  using namespace k3samd_kern;
  const int passes = o.passes, inject = o.inject;
  DevBuf<long long> d_report;
  HIP_CHECK(d_report.alloc(sizeof(long long) * kMemReportLen));
  if (o.do_check) {
    int rc = mem_selftest(d_report);
    if (rc) return rc;
  }

  size_t bytes = (size_t)o.mib << 20;
  if (o.vram_percent > 0) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    bytes =
        (free_b / 100 * (size_t)o.vram_percent) & ~((size_t)(1 << 20) - 1);
  }
  const int64_t n_cells = (int64_t)(bytes / 16);
  if (n_cells < kMemLogSlots) {
    std::fprintf(stderr, "mi-stream: memtest buffer too small\n");
    return 2;
  }
  DevBuf<void> buf;
  HIP_CHECK(buf.alloc(bytes));
  EventTimer timer;
  if (mem_report_reset(d_report)) return 1;

  std::printf("memtest: %.1f MiB, %d pass(es)%s\n", bytes / 1048576.0, passes,
              inject ? " [fault injection ON]" : "");
  std::printf("+------+--------------------------------+------------+\n");
  std::printf("| pass | march step                     |       GB/s |\n");
  std::printf("+------+--------------------------------+------------+\n");
  double verify_ms = 0;
  for (int p = 0; p < passes; ++p) {
    const uint64_t s = (uint64_t)p;
    const MemSpec addr{s, kMemPatternAddr, 0}, naddr{s, kMemPatternAddr, 1},
        walk{s, kMemPatternWalk, 0}, chk{s, kMemPatternChecker, 0};
    struct Step {
      const char* name;
      const MemSpec* from;
      const MemSpec* to;
    } steps[] = {
        {"fill ADDR", nullptr, &addr},
        {"verify ADDR   -> fill ~ADDR", &addr, &naddr},
        {"verify ~ADDR  -> fill WALK", &naddr, &walk},
        {"verify WALK   -> fill CHECKER", &walk, &chk},
        {"verify CHECKER", &chk, nullptr},
    };
    for (const Step& st : steps) {
      float ms;  // one timed launch, no warm-up
      if (timer.best_of(0, 1, [&](bool) {
            if (!st.from)
              launch_mem_fill(0, buf, n_cells, 0, *st.to, true);
            else if (!st.to)
              launch_mem_verify(0, buf, n_cells, 0, *st.from, d_report);
            else
              launch_mem_verify_fill(0, buf, n_cells, 0, *st.from, *st.to,
                                     d_report, true);
          }, &ms))
        return 1;
      const double moved = (st.from && st.to ? 2.0 : 1.0) * (double)bytes;
      if (st.from && !st.to) verify_ms += ms;
      std::printf("| %4d | %-30s | %10.1f |\n", p, st.name, gbps(moved, ms));
      if (!st.from && p == 0 && inject > 0) {
        // operator alerting drill: N single-bit flips at fixed cells
        for (int i = 0; i < inject; ++i)
          if (mem_flip(buf, 4ull * ((uint64_t)i * (n_cells / inject)),
                       1u << (i % 32)))
            return 1;
      }
    }
  }
  std::printf("+------+--------------------------------+------------+\n");

  HostMemReport r;
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  const bool clean = r.bad_dwords() == 0;
  const long long first_byte = clean ? -1 : (long long)(r.first() * 4);
  if (!clean) {
    std::printf("memtest: MISCOMPARE - %lld dword(s), %lld bit(s)\n",
                r.bad_dwords(), r.bad_bits());
    std::printf("%18s %10s %10s %10s\n", "byte offset", "expected", "actual",
                "xor");
    for (int i = 0; i < r.n_log(); ++i) {
      const long long* rec = r.log(i);
      std::printf("0x%016llx 0x%08x 0x%08x 0x%08x\n",
                  (unsigned long long)rec[0] * 4, (unsigned)rec[1],
                  (unsigned)rec[2], (unsigned)(rec[1] ^ rec[2]));
    }
  }
  std::printf(
      "{\"payload\": \"mi-memtest\", \"bytes\": %llu, \"passes\": %d, "
      "\"bad_dwords\": %lld, \"bad_bits\": %lld, \"first_bad_byte\": %lld, "
      "\"xor_or\": \"0x%08x\", \"verify_gbps\": %.1f, \"mem_clean\": %s}\n",
      (unsigned long long)bytes, passes, r.bad_dwords(), r.bad_bits(),
      first_byte, r.xor_or(),
      verify_ms > 0 ? gbps((double)bytes * passes, (float)verify_ms) : 0.0,
      clean ? "true" : "false");
  return clean ? 0 : 4;
}

// ---------------------------------------------------------------------------
// --gemmtest: verified bf16 MFMA GEMM (kernels in gemm_kernels.h) or, with
// --gemm-format, fp16 / int8 / fp32 / fp64 (gemm_dense_kernels.h). The
// operands are small integers, so C is known exactly and compared bitwise
// against a gold computed without the matrix pipes.
// Exit codes: 0 clean, 3 self-test / gold spot-check failed, 4 miscompare.
// ---------------------------------------------------------------------------

// Host-side operand dump (no HIP call): ROWS lines of COLS integers, the
// logical window gemm_operand(seed, which, ROW0 + i, COL0 + j).
int gemm_operand_dump(char** a) {
  const int which = std::atoi(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const uint64_t row0 = std::strtoull(a[2], nullptr, 0);
  const uint64_t col0 = std::strtoull(a[3], nullptr, 0);
  const uint64_t rows = std::strtoull(a[4], nullptr, 0);
  const uint64_t cols = std::strtoull(a[5], nullptr, 0);
  if (which != 0 && which != 1) {
    std::fprintf(stderr, "mi-stream: operand WHICH must be 0 (A) or 1 (B)\n");
    return 2;
  }
  for (uint64_t i = 0; i < rows; ++i) {
    for (uint64_t j = 0; j < cols; ++j)
      std::printf("%s%d", j ? " " : "",
                  k3samd_kern::gemm_operand(seed, which, (uint32_t)(row0 + i),
                                            (uint32_t)(col0 + j)));
    std::printf("\n");
  }
  return 0;
}

// The bf16 problem of the driver in gemm_verify.h: bf16 A[M,K] and Bt[N,K]
// of small integers from gemm_pattern.h.
struct Bf16Problem {
  using Result = float;
  static constexpr int kPoison = 0xFF;  // NaN
  static constexpr const char* kTag = "gemmtest";
  static constexpr int64_t kSelftestK = 128;
  DevBuf<void> a, bt;
  int64_t m = 0, n = 0, k = 0;

  Bf16Problem fresh() const { return {}; }
  const char* label() const { return ""; }
  int alloc(int64_t m_, int64_t n_, int64_t k_) {
    m = m_, n = n_, k = k_;
    HIP_CHECK(a.alloc((size_t)m * k * 2));
    HIP_CHECK(bt.alloc((size_t)n * k * 2));
    return 0;
  }
  void fill(uint64_t seed) {
    k3samd_kern::launch_gemm_fill(0, a, 0, seed, m, k);
    k3samd_kern::launch_gemm_fill(0, bt, 1, seed, n, k);
  }
  void gemm(float* c, int* where) {
    k3samd_kern::launch_gemm_bf16_nt(0, a, bt, c, where, m, n, k);
  }
  void ref(float* gold) {
    k3samd_kern::launch_gemm_ref_int(0, a, bt, gold, m, n, k);
  }

  // Element (row, col) of the generator product as a host integer dot product.
  float host_elem(uint64_t seed, uint32_t row, uint32_t col) const {
    long long s = 0;
    for (int64_t kk = 0; kk < k; ++kk)
      s += (long long)k3samd_kern::gemm_operand(seed, 0, row, (uint32_t)kk) *
           k3samd_kern::gemm_operand(seed, 1, (uint32_t)kk, col);
    return (float)s;
  }
  // host operands once, then the integer product
  std::vector<float> host_product(uint64_t seed) const {
    using k3samd_kern::gemm_operand;
    std::vector<int> ha(m * k), hb(k * n);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t kk = 0; kk < k; ++kk)
        ha[i * k + kk] = gemm_operand(seed, 0, (uint32_t)i, (uint32_t)kk);
    for (int64_t kk = 0; kk < k; ++kk)
      for (int64_t j = 0; j < n; ++j)
        hb[kk * n + j] = gemm_operand(seed, 1, (uint32_t)kk, (uint32_t)j);
    std::vector<float> c(m * n);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = 0; j < n; ++j) {
        int s = 0;
        for (int64_t kk = 0; kk < k; ++kk) s += ha[i * k + kk] * hb[kk * n + j];
        c[i * n + j] = (float)s;
      }
    return c;
  }
  void print_product_verdict(long long bad_mfma, long long bad_gold) const {
    if (bad_mfma || bad_gold)
      std::printf("gemmtest selftest: FAIL (256x256x128 vs host product: %lld "
                  "MFMA element(s), %lld gold element(s) differ)\n",
                  bad_mfma, bad_gold);
    else
      std::printf("gemmtest selftest: 256x256x128 MFMA product and integer "
                  "gold match the host product exactly\n");
  }
};

// The fp16 / int8 / fp32 / fp64 problem: the same operands in the format's
// element type, C and gold in its result type (gemm_dense_kernels.h).
template <int kFmt, typename Result_>
struct DenseProblem {
  using Result = Result_;
  // -1 is a legitimate int32 product; 0x80808080 lies outside +-2^23
  static constexpr int kPoison = kFmt == k3samd_kern::kGemmFmtInt8 ? 0x80 : 0xFF;
  static constexpr const char* kTag = "gemmtest";
  static constexpr int64_t kSelftestK = 2 * k3samd_kern::gemm_dense_step_k(kFmt);
  DevBuf<void> a, bt;
  int64_t m = 0, n = 0, k = 0;

  DenseProblem fresh() const { return {}; }
  const char* label() const {
    using namespace k3samd_kern;
    return kFmt == kGemmFmtFp16   ? "fp16 "
           : kFmt == kGemmFmtInt8 ? "int8 "
           : kFmt == kGemmFmtFp32 ? "fp32 "
                                  : "fp64 ";
  }
  int alloc(int64_t m_, int64_t n_, int64_t k_) {
    m = m_, n = n_, k = k_;
    const size_t elem = k3samd_kern::gemm_dense_elem_bytes(kFmt);
    HIP_CHECK(a.alloc((size_t)m * k * elem));
    HIP_CHECK(bt.alloc((size_t)n * k * elem));
    return 0;
  }
  void fill(uint64_t seed) {
    k3samd_kern::launch_gemm_dense_fill(0, kFmt, a, 0, seed, m, k);
    k3samd_kern::launch_gemm_dense_fill(0, kFmt, bt, 1, seed, n, k);
  }
  void gemm(Result* c, int* where) {
    k3samd_kern::launch_gemm_dense_nt(0, kFmt, a, bt, c, where, m, n, k);
  }
  void ref(Result* gold) {
    k3samd_kern::launch_gemm_dense_ref_int(0, kFmt, a, bt, gold, m, n, k);
  }

  // The integer products are Bf16Problem's; only the result type differs.
  Result host_elem(uint64_t seed, uint32_t row, uint32_t col) const {
    Bf16Problem b;
    b.k = k;
    return (Result)(long long)b.host_elem(seed, row, col);
  }
  std::vector<Result> host_product(uint64_t seed) const {
    Bf16Problem b;
    b.m = m, b.n = n, b.k = k;
    const std::vector<float> f = b.host_product(seed);  // exact: <= 2^23
    std::vector<Result> c(f.size());
    for (size_t i = 0; i < f.size(); ++i) c[i] = (Result)(long long)f[i];
    return c;
  }
  void print_product_verdict(long long bad_mfma, long long bad_gold) const {
    const char* name = k3samd_kern::gemm_dense_fmt_name(kFmt);
    if (bad_mfma || bad_gold)
      std::printf("gemmtest selftest: FAIL (256x256x%lld %s vs host product: "
                  "%lld MFMA element(s), %lld gold element(s) differ)\n",
                  (long long)kSelftestK, name, bad_mfma, bad_gold);
    else
      std::printf("gemmtest selftest: 256x256x%lld %s MFMA product and integer "
                  "gold match the host product exactly\n",
                  (long long)kSelftestK, name);
  }
};

// `format` is the word of --gemm-format, null without the flag: only then
// does the JSON line carry it.
template <typename Problem>
int run_gemmtest_as(Problem p, const Options& o, const char* format) {
  GemmVerifyResult v;
  int rc = gemm_verify(p, o.gemm_m, o.gemm_n, o.gemm_k, o.gemm_iters,
                       o.gemm_seconds, o.gemm_inject, o.do_check, &v);
  if (rc) return rc;
  std::printf("{\"payload\": \"mi-gemmtest\", ");
  if (format) std::printf("\"format\": \"%s\", ", format);
  std::printf(
      "\"m\": %lld, \"n\": %lld, \"k\": %lld, "
      "\"iters\": %lld, \"bad_elems\": %lld, \"bad_bits\": %lld, "
      "\"first_bad_row\": %lld, \"first_bad_col\": %lld, "
      "\"first_bad_xcc\": %d, \"avg_tflops\": %.1f, \"gold_ms\": %.1f, "
      "\"max_temp_c\": %ld, \"max_power_w\": %.0f, \"compute_clean\": %s}\n",
      (long long)o.gemm_m, (long long)o.gemm_n, (long long)o.gemm_k, v.iters,
      v.report.bad_dwords(), v.report.bad_bits(), v.first_bad_row,
      v.first_bad_col, v.first_bad_xcc,
      v.tflops(o.gemm_m, o.gemm_n, o.gemm_k), v.gold_ms, v.max_temp_c, v.max_power_w, v.clean() ? "true" : "false");
  return v.clean() ? 0 : 4;
}

int run_gemmtest(const Options& o) {
  using namespace k3samd_kern;
  switch (o.gemm_format) {
    case kGemmFmtFp16:
      return run_gemmtest_as(DenseProblem<kGemmFmtFp16, float>{}, o, "fp16");
    case kGemmFmtInt8:
      return run_gemmtest_as(DenseProblem<kGemmFmtInt8, int32_t>{}, o, "int8");
    case kGemmFmtFp32:
      return run_gemmtest_as(DenseProblem<kGemmFmtFp32, float>{}, o, "fp32");
    case kGemmFmtFp64:
      return run_gemmtest_as(DenseProblem<kGemmFmtFp64, double>{}, o, "fp64");
    default:
      return run_gemmtest_as(Bf16Problem{}, o,
                             o.gemm_format == kNoGemmFormat ? nullptr : "bf16");
  }
}

// ---- STREAM modes ----

// --all-gpus: concurrent non-temporal triad on every visible GPU (the
// in-pod demonstration of the headline metric at amd.com/gpu: N): per-GPU
// buffers + stream, launches overlapped, one global wall-clock.
int run_all_gpus(const Options& o, int ndev) {
  const int64_t n = o.mib * (1 << 20) / 4;
  const int64_t n4 = n / 4;
  const double step_bytes = 3.0 * n * 4;
  // Raw pointers with explicit per-device frees below, not DevBuf: a
  // DevBuf would free under whichever device is current when it dies.
  std::vector<f4*> A(ndev), B(ndev), C(ndev);
  std::vector<hipStream_t> streams(ndev);
  for (int d = 0; d < ndev; ++d) {
    HIP_CHECK(hipSetDevice(d));
    HIP_CHECK(hipMalloc(&A[d], n * 4));
    HIP_CHECK(hipMalloc(&B[d], n * 4));
    HIP_CHECK(hipMalloc(&C[d], n * 4));
    HIP_CHECK(hipMemset(B[d], 0x3c, n * 4));
    HIP_CHECK(hipMemset(C[d], 0x3d, n * 4));
    HIP_CHECK(hipStreamCreate(&streams[d]));
  }
  auto launch_all = [&] {
    for (int d = 0; d < ndev; ++d) {
      (void)hipSetDevice(d);
      k3samd_kern::launch_stream_triad(streams[d], A[d], B[d], C[d], kScalar,
                                       n4, true);
    }
  };
  auto sync_all = [&] {
    for (int d = 0; d < ndev; ++d) (void)hipStreamSynchronize(streams[d]);
  };
  for (int w = 0; w < 3; ++w) launch_all();
  sync_all();
  const auto t0 = Clock::now();
  for (int it = 0; it < o.iters; ++it) launch_all();
  sync_all();
  const double sec = seconds_since(t0);
  const double agg = ndev * step_bytes * o.iters / sec / 1e9;
  std::printf("mi-stream all-gpus: %d GPU(s) x %lld MiB, aggregate triad "
              "%.1f GB/s (%.1f per GPU)\n",
              ndev, (long long)o.mib, agg, agg / ndev);
  std::printf("{\"payload\": \"mi-stream\", \"mode\": \"all-gpus\", "
              "\"n_gpus\": %d, \"aggregate_triad_gbps\": %.1f}\n",
              ndev, agg);
  for (int d = 0; d < ndev; ++d) {
    (void)hipSetDevice(d);
    (void)hipFree(A[d]); (void)hipFree(B[d]); (void)hipFree(C[d]);
    (void)hipStreamDestroy(streams[d]);
  }
  return 0;
}

// The three fp32 buffers of --mib MiB each that the single-GPU STREAM
// modes work on (a = f(b, c)), and the timer they share.
struct StreamBufs {
  DevBuf<f4> a, b, c;
  int64_t n4 = 0;
  double bytes = 0;  // of one buffer
  EventTimer timer;

  int init(int64_t mib) {
    const int64_t n = mib * (1 << 20) / 4;  // fp32 elements
    n4 = n / 4;
    bytes = (double)n * 4;
    HIP_CHECK(a.alloc((size_t)n * 4));
    HIP_CHECK(b.alloc((size_t)n * 4));
    HIP_CHECK(c.alloc((size_t)n * 4));
    HIP_CHECK(hipMemset(b, 0x3c, (size_t)n * 4));
    HIP_CHECK(hipMemset(c, 0x3d, (size_t)n * 4));
    return 0;
  }
};

// --lds-compare: direct-nt vs LDS-staged triad (SURVEY §2c blueprint
// comparison). 1 warm-up, best of --iters.
int run_lds_compare(const Options& o, StreamBufs& s) {
  using namespace k3samd_kern;
  float direct_ms, lds_ms;
  if (s.timer.best_of(1, o.iters, [&](bool) {
        launch_stream_triad(0, s.a, s.b, s.c, kScalar, s.n4, true);
      }, &direct_ms) ||
      s.timer.best_of(1, o.iters, [&](bool) {
        launch_stream_triad_lds(0, s.a, s.b, s.c, kScalar, s.n4);
      }, &lds_ms))
    return 1;
  const double direct = gbps(3 * s.bytes, direct_ms);
  const double lds = gbps(3 * s.bytes, lds_ms);
  std::printf("triad %lld MiB: direct-nt %.1f GB/s | LDS-staged %.1f GB/s "
              "(%.1f%%)\n",
              (long long)o.mib, direct, lds, 100.0 * lds / direct);
  std::printf("{\"payload\": \"mi-stream-lds\", \"direct_gbps\": %.1f, "
              "\"lds_staged_gbps\": %.1f}\n", direct, lds);
  return 0;
}

// --tune: sweep block-size x unroll x grid-occupancy for the grid-stride
// non-temporal triad; prints GB/s per config (exploration tool). These are
// the one set of STREAM launches with an explicit (blocks, tpb) grid.
// 2 warm-ups, best of --iters.
int run_tune(const Options& o, StreamBufs& s) {
  using namespace k3samd_kern;
  f4 *a = s.a, *b = s.b, *c = s.c;
  std::printf("tune: grid-stride nt triad, %lld MiB buffers\n",
              (long long)o.mib);
  std::printf("%8s %6s %8s %10s\n", "tpb", "unroll", "blocks", "GB/s");
  for (int tpb : {256, 512, 1024}) {
    for (int wavesper : {4, 8, 16, 32}) {  // blocks = CUs*waves*64/tpb
      const int blocks = 256 * wavesper * 64 / tpb;
      double rate[3];
      int u = 0;
      for (auto kern : {stream_triad_gs_kernel<true, 1>,
                        stream_triad_gs_kernel<true, 2>,
                        stream_triad_gs_kernel<true, 4>}) {
        float ms;
        if (s.timer.best_of(2, o.iters, [&](bool) {
              hipLaunchKernelGGL(kern, dim3(blocks), dim3(tpb), 0, 0, a, b, c,
                                 kScalar, s.n4);
            }, &ms))
          return 1;
        rate[u++] = gbps(3 * s.bytes, ms);
      }
      std::printf("%8d %6d %8d  U1 %8.1f U2 %8.1f U4 %8.1f\n", tpb, 1, blocks,
                  rate[0], rate[1], rate[2]);
    }
  }
  return 0;
}

// --burn: saturate HBM (nt triad) and the matrix pipes (bf16 MFMA)
// concurrently on two streams for --burn seconds, sampling thermals from
// sysfs. Node-acceptance analog of gpu-burn.
int run_burn(const Options& o, StreamBufs& s) {
  using namespace k3samd_kern;
  hipStream_t s_mem, s_mfma;
  HIP_CHECK(hipStreamCreate(&s_mem));
  HIP_CHECK(hipStreamCreate(&s_mfma));
  const int mf_blocks = 1024, mf_iters = 512;
  DevBuf<float> mf_out;
  HIP_CHECK(mf_out.alloc(mf_blocks * sizeof(float)));
  const double triad_bytes = 3.0 * s.bytes;
  const double mf_flops =
      mfma_throughput_flops(kMfmaBf16_16x16x32, mf_blocks, mf_iters);
  ThermalSampler thermal;
  const auto t_end = Clock::now() + std::chrono::seconds(o.burn_s);
  // RAS snapshot before the stress: ECC errors that APPEAR during the
  // burn are the node-acceptance failure signal
  k3samd::GpuHealthCounters ras0 =
      k3samd::read_gpu_health(k3samd::default_sysfs_root(), thermal.card);
  uint64_t launches = 0, launches_last = 0;  // of each of the two kernels
  std::printf("burn: %d s of concurrent HBM streaming + bf16 MFMA\n",
              o.burn_s);
  std::printf("%6s %12s %12s %6s %7s %6s\n", "t(s)", "GB/s", "TFLOP/s",
              "temp", "power", "busy");
  const auto t0 = Clock::now();
  auto next_report = t0 + std::chrono::seconds(2);
  auto t_last = t0;
  while (Clock::now() < t_end) {
    for (int i = 0; i < 8; ++i) {
      launch_stream_triad(s_mem, s.a, s.b, s.c, kScalar, s.n4, true);
      launch_mfma_throughput(s_mfma, kMfmaBf16_16x16x32, mf_out, mf_blocks,
                             mf_iters);
      ++launches;
    }
    HIP_CHECK(hipStreamSynchronize(s_mem));
    HIP_CHECK(hipStreamSynchronize(s_mfma));
    if (Clock::now() >= next_report) {
      const auto st = thermal.sample();
      const double dt = seconds_since(t_last);
      const uint64_t n = launches - launches_last;
      std::printf("%6.0f %12.1f %12.1f %s %5ld%%\n", seconds_since(t0),
                  n * triad_bytes / dt / 1e9, n * mf_flops / dt / 1e12,
                  thermal.cells, st.busy_percent);
      std::fflush(stdout);
      launches_last = launches;
      t_last = Clock::now();
      next_report += std::chrono::seconds(2);
    }
  }
  const double total_s = seconds_since(t0);
  k3samd::GpuHealthCounters ras1 =
      k3samd::read_gpu_health(k3samd::default_sysfs_root(), thermal.card);
  long d_ue = (ras0.ras_ue >= 0 && ras1.ras_ue >= 0)
                  ? ras1.ras_ue - ras0.ras_ue : -1;
  long d_ce = (ras0.ras_ce >= 0 && ras1.ras_ce >= 0)
                  ? ras1.ras_ce - ras0.ras_ce : -1;
  bool ras_clean = d_ue <= 0 && d_ce <= 0;
  if (ras0.ras_present)
    std::printf("burn RAS delta: ue %+ld ce %+ld (%s)\n", d_ue, d_ce,
                ras_clean ? "clean" : "ERRORS DURING BURN");
  std::printf(
      "{\"payload\": \"mi-burn\", \"seconds\": %.0f, \"avg_triad_gbps\": "
      "%.1f, \"avg_mfma_tflops\": %.1f, \"max_temp_c\": %ld, "
      "\"max_power_w\": %.0f, \"ras_delta_ue\": %ld, "
      "\"ras_delta_ce\": %ld, \"ras_clean\": %s}\n",
      total_s, launches * triad_bytes / total_s / 1e9,
      launches * mf_flops / total_s / 1e12, thermal.max_temp_c,
      thermal.max_power_w, d_ue, d_ce, ras_clean ? "true" : "false");
  HIP_CHECK(hipStreamDestroy(s_mem));
  HIP_CHECK(hipStreamDestroy(s_mfma));
  return 0;
}

// Default mode: the STREAM table (2 warm-ups, best of --iters per cell),
// the MFMA rows (1 warm-up at 256 iterations, best of 3: rides out the
// clock ramp) and the JSON line.
int run_stream_table(const Options& o, StreamBufs& s,
                     const hipDeviceProp_t& prop) {
  using namespace k3samd_kern;
  struct Row {
    const char* name;
    double bytes;
    float best_ms[2];  // plain, non-temporal
  } rows[] = {{"copy", 2 * s.bytes, {}}, {"scale", 2 * s.bytes, {}},
              {"add", 3 * s.bytes, {}}, {"triad", 3 * s.bytes, {}}};
  auto launch = [&](int op, bool nt) {
    switch (op) {
      case 0: return launch_stream_copy(0, s.a, s.b, s.n4, nt);
      case 1: return launch_stream_scale(0, s.a, s.c, kScalar, s.n4, nt);
      case 2: return launch_stream_add(0, s.a, s.b, s.c, s.n4, nt);
      default: return launch_stream_triad(0, s.a, s.b, s.c, kScalar, s.n4, nt);
    }
  };
  for (int op = 0; op < 4; ++op)
    for (int nt = 0; nt < 2; ++nt)
      if (s.timer.best_of(2, o.iters, [&](bool) { launch(op, nt); },
                          &rows[op].best_ms[nt]))
        return 1;

  std::printf("+--------+-------------------+-------------------+\n");
  std::printf("| STREAM | plain GB/s        | non-temporal GB/s |\n");
  std::printf("+--------+-------------------+-------------------+\n");
  for (const Row& r : rows)
    std::printf("| %-6s | %17.1f | %17.1f |\n", r.name,
                gbps(r.bytes, r.best_ms[0]), gbps(r.bytes, r.best_ms[1]));
  std::printf("+--------+-------------------+-------------------+\n");

  double mfma_tf = 0;
  if (o.do_mfma) {
    // 4096 blocks + 4 chains measured best (tools/mfma_tune.hip sweep:
    // 2477 TF = 99 % of the 2.5 PF dense peak)
    const int blocks = 4096, mf_iters = 4096;
    DevBuf<float> out;
    HIP_CHECK(out.alloc(blocks * sizeof(float)));
    const MfmaKind kinds[5] = {kMfmaBf16_16x16x32, kMfmaBf16_32x32x16,
                               kMfmaMxFp8, kMfmaMxFp6, kMfmaMxFp4};
    double tf[5];
    for (int i = 0; i < 5; ++i) {
      float ms;
      if (s.timer.best_of(1, 3, [&](bool warm) {
            launch_mfma_throughput(0, kinds[i], out, blocks,
                                   warm ? 256 : mf_iters);
          }, &ms))
        return 1;
      tf[i] = tflops(mfma_throughput_flops(kinds[i], blocks, mf_iters), ms);
    }
    std::printf("| MFMA bf16 16x16x32: %7.1f TF | 32x32x16: %7.1f TF     |\n",
                tf[0], tf[1]);
    std::printf("| MFMA MX 16x16x128  fp8: %6.1f | fp6: %6.1f | fp4: %6.1f |\n",
                tf[2], tf[3], tf[4]);
    std::printf("+--------+-------------------+-------------------+\n");
    mfma_tf = std::max(tf[0], tf[1]);
  }

  const Row& triad = rows[3];
  std::printf(
      "{\"payload\": \"mi-stream\", \"gpu\": \"%s\", \"arch\": \"%s\", "
      "\"buffer_MiB\": %lld, \"triad_gbps\": %.1f, \"mfma_bf16_tflops\": "
      "%.1f}\n",
      prop.name, prop.gcnArchName, (long long)o.mib,
      gbps(triad.bytes, std::min(triad.best_ms[0], triad.best_ms[1])),
      mfma_tf);
  return 0;
}

// ---- command line ----

const char kUsage[] =
    "mi-stream [--mib N] [--iters N] [--device D] [--no-mfma]"
    " [--tune] [--lds-compare] [--all-gpus] [--burn SECONDS]"
    " [--memtest [--passes N] [--vram-percent P]"
    " [--memtest-inject N]] [--memtest-pattern-dump PATTERN"
    " SEED INVERT CELL_OFFSET N_CELLS]"
    " [--gemmtest [--gemm-size S | --gemm-mnk M N K]"
    " [--gemm-iters I | --gemm-seconds T] [--gemm-inject N]]"
    " [--gemm-operand-dump WHICH SEED ROW0 COL0 ROWS COLS]\n";

// The usage line is pinned byte for byte by the CLI tests, so like
// --no-check, --gemm-format (bf16|fp16|int8|fp32|fp64) is not on it: the
// README, the runbook and the refusal of an unknown format name it.
// Flags are matched left to right. The two dump flags run (host only) and
// return as soon as they are reached; an unknown flag, or a flag short of
// its values, prints the usage line and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    const FlagMatcher flag{argc, argv, i};
    if (flag("--mib", 1)) o.mib = std::atoll(argv[++i]);
    else if (flag("--iters", 1)) o.iters = std::atoi(argv[++i]);
    else if (flag("--device", 1)) o.device = std::atoi(argv[++i]);
    else if (flag("--no-mfma")) o.do_mfma = false;
    else if (flag("--no-check")) o.do_check = false;
    else if (flag("--tune")) o.tune = true;
    else if (flag("--lds-compare")) o.lds_compare = true;
    else if (flag("--all-gpus")) o.all_gpus = true;
    else if (flag("--burn", 1)) o.burn_s = std::atoi(argv[++i]);
    else if (flag("--memtest")) o.memtest = true;
    else if (flag("--passes", 1)) o.passes = std::atoi(argv[++i]);
    else if (flag("--vram-percent", 1)) o.vram_percent = std::atoi(argv[++i]);
    else if (flag("--memtest-inject", 1)) o.inject = std::atoi(argv[++i]);
    else if (flag("--memtest-pattern-dump", 5))
      return mem_pattern_dump(argv + i + 1);
    else if (flag("--gemmtest")) o.gemmtest = true;
    else if (flag("--gemm-size", 1))
      o.gemm_m = o.gemm_n = o.gemm_k = std::atoll(argv[++i]);
    else if (flag("--gemm-mnk", 3)) {
      o.gemm_m = std::atoll(argv[++i]);
      o.gemm_n = std::atoll(argv[++i]);
      o.gemm_k = std::atoll(argv[++i]);
    } else if (flag("--gemm-iters", 1)) o.gemm_iters = std::atoi(argv[++i]);
    else if (flag("--gemm-seconds", 1)) o.gemm_seconds = std::atoi(argv[++i]);
    else if (flag("--gemm-inject", 1)) o.gemm_inject = std::atoi(argv[++i]);
    else if (flag("--gemm-format", 1)) {
      using namespace k3samd_kern;
      const char* w = o.gemm_format_bad = argv[++i];
      for (int f = 0; f <= kGemmFmtFp64; ++f)
        if (!std::strcmp(w, f ? gemm_dense_fmt_name(f) : "bf16")) {
          o.gemm_format = f;
          o.gemm_format_bad = nullptr;
        }
    } else if (flag("--gemm-operand-dump", 6))
      return gemm_operand_dump(argv + i + 1);
    else return usage_status(kUsage, argv[i]);
  }
  return kRun;
}

// Range checks of the chosen mode, before any HIP call. Returns 0 or the
// exit status 2. Also applies the --gemmtest default of one second.
int validate_options(Options& o) {
  if (o.memtest &&
      (o.passes < 1 || o.mib < 1 || o.inject < 0 || o.inject > 16 ||
       (o.vram_percent != 0 && (o.vram_percent < 1 || o.vram_percent > 90)))) {
    std::fprintf(stderr, "mi-stream: --memtest needs --passes >= 1, --mib >= 1,"
                         " --vram-percent 1..90, --memtest-inject 1..16\n");
    return 2;
  }
  if (o.gemmtest) {
    if (o.gemm_iters == 0 && o.gemm_seconds == 0) o.gemm_seconds = 1;
    if (o.gemm_format_bad) {
      std::fprintf(stderr, "mi-stream: --gemm-format %s: the formats are bf16"
                           " (K-step 64), fp16 (64), int8 (128), fp32 (32),"
                           " fp64 (16)\n", o.gemm_format_bad);
      return 2;
    }
    if (o.gemm_format > 0) {  // a dense format: its own K-step
      using namespace k3samd_kern;
      if (!gemm_dense_shape_ok(o.gemm_format, o.gemm_m, o.gemm_n, o.gemm_k) ||
          o.gemm_k > kGemmExactMaxK || o.gemm_iters < 0 ||
          o.gemm_seconds < 0 || (o.gemm_iters > 0 && o.gemm_seconds > 0) ||
          o.gemm_inject < 0 || o.gemm_inject > 16) {
        std::fprintf(stderr, "mi-stream: --gemmtest --gemm-format %s needs M"
                             " and N multiples of 128, K a multiple of %d and"
                             " <= 32768, one of --gemm-iters >= 1 /"
                             " --gemm-seconds >= 1, --gemm-inject 1..16\n",
                     gemm_dense_fmt_name(o.gemm_format),
                     gemm_dense_step_k(o.gemm_format));
        return 2;
      }
    } else if (!k3samd_kern::gemm_shape_ok(o.gemm_m, o.gemm_n, o.gemm_k) ||
        o.gemm_k > k3samd_kern::kGemmExactMaxK || o.gemm_iters < 0 ||
        o.gemm_seconds < 0 || (o.gemm_iters > 0 && o.gemm_seconds > 0) ||
        o.gemm_inject < 0 || o.gemm_inject > 16) {
      std::fprintf(stderr, "mi-stream: --gemmtest needs M and N multiples of"
                           " 128, K a multiple of 64 and <= 32768, one of"
                           " --gemm-iters >= 1 / --gemm-seconds >= 1,"
                           " --gemm-inject 1..16\n");
      return 2;
    }
  }
  return 0;
}

}  // namespace

// Exit status: 0 ok, 1 HIP error, 2 usage, 3 an oracle/self-test failed,
// 4 memtest or gemmtest data miscompare.
int main(int argc, char** argv) {
  Options o;
  int rc = parse_options(argc, argv, o);
  if (rc != kRun) return rc;
  if ((rc = validate_options(o)) != 0) return rc;

  // --all-gpus counts the devices and selects none here
  int ndev = 0;
  hipDeviceProp_t prop;
  if (open_device(o.device, &ndev, o.all_gpus ? nullptr : &prop)) return 1;

  // When several mode flags are given, the first in this order wins:
  // all-gpus, memtest, gemmtest, lds-compare, tune, burn, then the default
  // table. The order is the one the modes have always had.
  if (o.all_gpus) {
    if (o.do_check && !self_check()) return 3;  // oracle on device 0 first
    return run_all_gpus(o, ndev);
  }

  std::printf("mi-stream: %s (%s), %d visible GPU(s), %d CUs, %.0f GiB VRAM\n",
              prop.name, prop.gcnArchName, ndev, prop.multiProcessorCount,
              (double)prop.totalGlobalMem / (1 << 30));
  // these two run their own self-tests (unless --no-check)
  if (o.memtest) return run_memtest(o);
  if (o.gemmtest) return run_gemmtest(o);

  if (o.do_check && !self_check()) return 3;  // pod log is the oracle
  StreamBufs s;
  if (s.init(o.mib)) return 1;
  if (o.lds_compare) return run_lds_compare(o, s);
  if (o.tune) return run_tune(o, s);
  if (o.burn_s > 0) return run_burn(o, s);
  return run_stream_table(o, s, prop);
}
