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
// Build: hipcc --offload-arch=gfx950 -O3 mi_stream.hip -o mi-stream

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../k3samd/ops/hip/gemm_kernels.h"
#include "../../k3samd/ops/hip/memtest_kernels.h"
#include "../../k3samd/ops/hip/stream_kernels.h"
#include "../topology/gpu_health.h"
#include "../topology/kfd_topology.h"

#define HIP_CHECK(x)                                                         \
  do {                                                                       \
    hipError_t err_ = (x);                                                   \
    if (err_ != hipSuccess) {                                                \
      std::fprintf(stderr, "mi-stream: %s failed: %s\n", #x,                 \
                   hipGetErrorString(err_));                                 \
      return 1;                                                              \
    }                                                                        \
  } while (0)

using k3samd_kern::f4;

namespace {

struct Timing {
  float best_ms = 1e30f;
};

double gbps(double bytes, float ms) { return bytes / (ms * 1e6); }

// Numerics self-check: the pod log doubles as a correctness oracle (the
// reference's nvidia-smi output carried version oracles the same way,
// /root/reference/README.md:139-147). Three checks against host-computed
// references: fp32 triad (exact), one bf16 MFMA tile, one block-scaled
// MX-fp8 tile (identity-A => must reproduce B exactly).
bool self_check() {
  using namespace k3samd_kern;
  bool ok = true;
  // --- triad, 4096 elements, exactly-representable values
  {
    const int64_t n = 4096, n4 = n / 4;
    float *a, *b, *c;
    (void)hipMalloc(&a, n * 4);
    (void)hipMalloc(&b, n * 4);
    (void)hipMalloc(&c, n * 4);
    std::vector<float> hb(n), hc(n), ha(n);
    for (int64_t i = 0; i < n; ++i) {
      hb[i] = (float)((i % 31) - 15);
      hc[i] = (float)((i % 17) - 8) * 0.5f;
    }
    (void)hipMemcpy(b, hb.data(), n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(c, hc.data(), n * 4, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(stream_triad_kernel<true>, dim3(stream_grid(n4)),
                       dim3(kThreadsPerBlock), 0, 0, (f4*)a, (f4*)b, (f4*)c,
                       2.5f, n4);
    (void)hipMemcpy(ha.data(), a, n * 4, hipMemcpyDeviceToHost);
    for (int64_t i = 0; i < n && ok; ++i)
      if (ha[i] != hb[i] + 2.5f * hc[i]) ok = false;
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
    if (!ok) { std::printf("numerics: triad FAIL\n"); return false; }
  }
#if 1
  // --- bf16 MFMA tile vs host float reference
  double mfma_err = 0;
  {
    uint16_t *A, *B; float* D;
    (void)hipMalloc(&A, 16 * 32 * 2);
    (void)hipMalloc(&B, 32 * 16 * 2);
    (void)hipMalloc(&D, 16 * 16 * 4);
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
    hipLaunchKernelGGL(mfma_gemm16_kernel, dim3(1), dim3(64), 0, 0, A, B, D,
                       0);
    std::vector<float> hD(256);
    (void)hipMemcpy(hD.data(), D, 256 * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        float ref = 0;
        for (int k = 0; k < 32; ++k) ref += fA[i * 32 + k] * fB[k * 16 + j];
        double e = std::abs(hD[i * 16 + j] - ref);
        if (e > mfma_err) mfma_err = e;
      }
    (void)hipFree(A); (void)hipFree(B); (void)hipFree(D);
    if (mfma_err > 1e-3) {
      std::printf("numerics: bf16 MFMA FAIL (err %g)\n", mfma_err);
      return false;
    }
  }
  // --- MX-fp8 identity tile: D must equal B rows exactly
  double mx_err = 0;
  {
    uint8_t *A, *B; float* D;
    (void)hipMalloc(&A, 16 * 128);
    (void)hipMalloc(&B, 16 * 128);
    (void)hipMalloc(&D, 16 * 16 * 4);
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
    hipLaunchKernelGGL(mx_gemm16_kernel<0>, dim3(1), dim3(64), 0, 0, A, B, D);
    std::vector<float> hD(256);
    (void)hipMemcpy(hD.data(), D, 256 * 4, hipMemcpyDeviceToHost);
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        double e = std::abs(hD[i * 16 + j] - fB[i * 16 + j]);
        if (e > mx_err) mx_err = e;
      }
    (void)hipFree(A); (void)hipFree(B); (void)hipFree(D);
    if (mx_err != 0.0) {
      std::printf("numerics: MX-fp8 FAIL (err %g)\n", mx_err);
      return false;
    }
  }
  std::printf(
      "numerics: triad exact, bf16 MFMA err %.2g, MX-fp8 identity exact\n",
      mfma_err);
#endif
  return true;
}

// ---------------------------------------------------------------------------
// --memtest: HBM pattern memory test (kernels in memtest_kernels.h).
// Exit codes: 0 clean, 3 detector self-test failed, 4 data miscompare.
// ---------------------------------------------------------------------------

struct HostMemReport {
  long long v[k3samd_kern::kMemReportLen];
  long long bad_dwords() const { return v[0]; }
  long long bad_bits() const { return v[1]; }
  unsigned long long first() const { return (unsigned long long)v[2]; }
  unsigned xor_or() const { return (unsigned)v[3]; }
  int n_log() const {
    return v[4] > k3samd_kern::kMemLogSlots ? k3samd_kern::kMemLogSlots
                                            : (int)v[4];
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

// Detector self-test: a detector that has never fired proves nothing.
// Fill 1 MiB, flip three known bits, verify, and require exactly those
// three dwords/bits (count, first index, xor-or and log) to come back.
// Returns 0 ok, 3 detector failed, 1 HIP error.
int mem_selftest(void* d_report) {
  using namespace k3samd_kern;
  const int64_t n_cells = (1 << 20) / 16;
  const MemSpec spec{0x5EEDF00Dull, kMemPatternAddr, 0};
  void* buf;
  HIP_CHECK(hipMalloc(&buf, n_cells * 16));
  launch_mem_fill(0, buf, n_cells, 0, spec, true);
  HIP_CHECK(hipDeviceSynchronize());
  const uint64_t g[3] = {0, 4ull * 12345 + 2, 4ull * n_cells - 1};
  const uint32_t mask[3] = {1u << 0, 1u << 17, 1u << 31};
  for (int i = 0; i < 3; ++i)
    if (mem_flip(buf, g[i], mask[i])) return 1;
  if (mem_report_reset(d_report)) return 1;
  launch_mem_verify(0, buf, n_cells, 0, spec, d_report);
  HIP_CHECK(hipGetLastError());
  HostMemReport r;
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(buf));
  int caught = 0;
  for (int i = 0; i < 3; ++i) {
    const uint32_t expect = memtest_cell(spec, g[i] / 4).d[g[i] % 4];
    for (int s = 0; s < r.n_log(); ++s) {
      const long long* rec = r.v + kMemReportHeader + 3 * s;
      if ((uint64_t)rec[0] == g[i] && (uint32_t)rec[1] == expect &&
          (uint32_t)rec[2] == (expect ^ mask[i])) {
        ++caught;
        break;
      }
    }
  }
  bool ok = caught == 3 && r.bad_dwords() == 3 && r.bad_bits() == 3 &&
            r.first() == g[0] && r.v[4] == 3 &&
            r.xor_or() == (mask[0] | mask[1] | mask[2]);
  if (!ok) {
    std::printf("memtest selftest: FAIL (caught %d/3, bad_dwords %lld, "
                "bad_bits %lld, xor_or 0x%08x)\n",
                caught, r.bad_dwords(), r.bad_bits(), r.xor_or());
    return 3;
  }
  std::printf("memtest selftest: detector caught 3/3 injected flips\n");
  return 0;
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

int run_memtest(int64_t mib, int vram_percent, int passes, int inject,
                bool do_check) {
  using namespace k3samd_kern;
  void* d_report;
  HIP_CHECK(hipMalloc(&d_report, sizeof(long long) * kMemReportLen));
  if (do_check) {
    int rc = mem_selftest(d_report);
    if (rc) return rc;
  }

  size_t bytes = (size_t)mib << 20;
  if (vram_percent > 0) {
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    bytes = (free_b / 100 * (size_t)vram_percent) & ~((size_t)(1 << 20) - 1);
  }
  const int64_t n_cells = (int64_t)(bytes / 16);
  if (n_cells < kMemLogSlots) {
    std::fprintf(stderr, "mi-stream: memtest buffer too small\n");
    return 2;
  }
  void* buf;
  HIP_CHECK(hipMalloc(&buf, bytes));
  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
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
      HIP_CHECK(hipEventRecord(ev0));
      if (!st.from)
        launch_mem_fill(0, buf, n_cells, 0, *st.to, true);
      else if (!st.to)
        launch_mem_verify(0, buf, n_cells, 0, *st.from, d_report);
      else
        launch_mem_verify_fill(0, buf, n_cells, 0, *st.from, *st.to, d_report,
                               true);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(ev1));
      HIP_CHECK(hipEventSynchronize(ev1));
      float ms;
      HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
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
      const long long* rec = r.v + kMemReportHeader + 3 * i;
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
  HIP_CHECK(hipFree(buf));
  HIP_CHECK(hipFree(d_report));
  return clean ? 0 : 4;
}

// ---------------------------------------------------------------------------
// --gemmtest: verified bf16 MFMA GEMM (kernels in gemm_kernels.h). The
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

// Element (m, n) of the generator product as a host integer dot product.
long long gemm_host_dot(uint64_t seed, uint32_t m, uint32_t n, int64_t k) {
  long long s = 0;
  for (int64_t kk = 0; kk < k; ++kk)
    s += (long long)k3samd_kern::gemm_operand(seed, 0, m, (uint32_t)kk) *
         k3samd_kern::gemm_operand(seed, 1, (uint32_t)kk, n);
  return s;
}

struct GemmBufs {
  void *a = nullptr, *bt = nullptr, *c = nullptr, *gold = nullptr;
  int* where = nullptr;
  int64_t tiles = 0;
};

int gemm_alloc(GemmBufs& g, int64_t m, int64_t n, int64_t k) {
  g.tiles = (m / k3samd_kern::kGemmBM) * (n / k3samd_kern::kGemmBN);
  HIP_CHECK(hipMalloc(&g.a, (size_t)m * k * 2));
  HIP_CHECK(hipMalloc(&g.bt, (size_t)n * k * 2));
  HIP_CHECK(hipMalloc(&g.c, (size_t)m * n * 4));
  HIP_CHECK(hipMalloc(&g.gold, (size_t)m * n * 4));
  HIP_CHECK(hipMalloc(&g.where, (size_t)g.tiles * 8));
  HIP_CHECK(hipMemset(g.c, 0xFF, (size_t)m * n * 4));  // NaN: unwritten != gold
  HIP_CHECK(hipMemset(g.where, 0xFF, (size_t)g.tiles * 8));
  return 0;
}

int gemm_free(GemmBufs& g) {
  HIP_CHECK(hipFree(g.a));
  HIP_CHECK(hipFree(g.bt));
  HIP_CHECK(hipFree(g.c));
  HIP_CHECK(hipFree(g.gold));
  HIP_CHECK(hipFree(g.where));
  return 0;
}

// Self-test: (1) a 256x256x128 product, both the MFMA result and the
// integer gold, against the host integer product of gemm_pattern.h;
// (2) the detector drill of mem_selftest on C: flip three known bits,
// require exactly those three back. Returns 0 ok, 3 failed, 1 HIP error.
int gemm_selftest(void* d_report) {
  using namespace k3samd_kern;
  const int64_t m = 256, n = 256, k = 128;
  const uint64_t seed = 0x5EEDF00Dull;
  GemmBufs g;
  if (gemm_alloc(g, m, n, k)) return 1;
  launch_gemm_fill(0, g.a, 0, seed, m, k);
  launch_gemm_fill(0, g.bt, 1, seed, n, k);
  launch_gemm_ref_int(0, g.a, g.bt, g.gold, m, n, k);
  launch_gemm_bf16_nt(0, g.a, g.bt, g.c, g.where, m, n, k);
  HIP_CHECK(hipGetLastError());
  std::vector<float> hc(m * n), hg(m * n);
  HIP_CHECK(hipMemcpy(hc.data(), g.c, hc.size() * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hg.data(), g.gold, hg.size() * 4, hipMemcpyDeviceToHost));
  // host operands once, then the integer product
  std::vector<int> ha(m * k), hb(k * n);
  for (int64_t i = 0; i < m; ++i)
    for (int64_t kk = 0; kk < k; ++kk)
      ha[i * k + kk] = gemm_operand(seed, 0, (uint32_t)i, (uint32_t)kk);
  for (int64_t kk = 0; kk < k; ++kk)
    for (int64_t j = 0; j < n; ++j)
      hb[kk * n + j] = gemm_operand(seed, 1, (uint32_t)kk, (uint32_t)j);
  long long bad_mfma = 0, bad_gold = 0;
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < n; ++j) {
      int s = 0;
      for (int64_t kk = 0; kk < k; ++kk) s += ha[i * k + kk] * hb[kk * n + j];
      if (hc[i * n + j] != (float)s) ++bad_mfma;
      if (hg[i * n + j] != (float)s) ++bad_gold;
    }
  if (bad_mfma || bad_gold) {
    std::printf("gemmtest selftest: FAIL (256x256x128 vs host product: %lld "
                "MFMA element(s), %lld gold element(s) differ)\n",
                bad_mfma, bad_gold);
    return 3;
  }
  std::printf("gemmtest selftest: 256x256x128 MFMA product and integer gold "
              "match the host product exactly\n");

  const uint64_t e[3] = {0, 12345, (uint64_t)(m * n - 1)};
  const uint32_t mask[3] = {1u << 0, 1u << 17, 1u << 31};
  for (int i = 0; i < 3; ++i)
    if (mem_flip(g.c, e[i], mask[i])) return 1;
  if (mem_report_reset(d_report)) return 1;
  launch_buf_compare(0, g.c, g.gold, m * n / 4, d_report);
  HIP_CHECK(hipGetLastError());
  HostMemReport r;
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  int caught = 0;
  for (int i = 0; i < 3; ++i) {
    uint32_t expect;
    std::memcpy(&expect, &hg[e[i]], 4);
    for (int s = 0; s < r.n_log(); ++s) {
      const long long* rec = r.v + kMemReportHeader + 3 * s;
      if ((uint64_t)rec[0] == e[i] && (uint32_t)rec[1] == expect &&
          (uint32_t)rec[2] == (expect ^ mask[i])) {
        ++caught;
        break;
      }
    }
  }
  if (gemm_free(g)) return 1;
  bool ok = caught == 3 && r.bad_dwords() == 3 && r.bad_bits() == 3 &&
            r.first() == e[0] && r.v[4] == 3 &&
            r.xor_or() == (mask[0] | mask[1] | mask[2]);
  if (!ok) {
    std::printf("gemmtest selftest: FAIL (caught %d/3, bad_elems %lld, "
                "bad_bits %lld, xor_or 0x%08x)\n",
                caught, r.bad_dwords(), r.bad_bits(), r.xor_or());
    return 3;
  }
  std::printf("gemmtest selftest: detector caught 3/3 injected flips\n");
  return 0;
}

// Element index of injected flip i of `inject` (documented: evenly spaced
// from element 0, bit i % 32).
uint64_t gemm_inject_elem(int i, int inject, int64_t m, int64_t n) {
  return (uint64_t)i * ((uint64_t)(m * n) / (uint64_t)inject);
}

int run_gemmtest(int64_t m, int64_t n, int64_t k, int iters, int seconds,
                 int inject, bool do_check) {
  using namespace k3samd_kern;
  const uint64_t seed = 0;
  void* d_report;
  HIP_CHECK(hipMalloc(&d_report, sizeof(long long) * kMemReportLen));
  if (do_check) {
    int rc = gemm_selftest(d_report);
    if (rc) return rc;
  }
  GemmBufs g;
  if (gemm_alloc(g, m, n, k)) return 1;
  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
  launch_gemm_fill(0, g.a, 0, seed, m, k);
  launch_gemm_fill(0, g.bt, 1, seed, n, k);
  HIP_CHECK(hipEventRecord(ev0));
  launch_gemm_ref_int(0, g.a, g.bt, g.gold, m, n, k);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(ev1));
  HIP_CHECK(hipEventSynchronize(ev1));
  float gold_ms;
  HIP_CHECK(hipEventElapsedTime(&gold_ms, ev0, ev1));

  // gold spot-check: 64 fixed elements against host integer dot products
  // of the generator — independent of the device entirely
  for (int i = 0; i < 64; ++i) {
    const uint32_t row = i == 63 ? (uint32_t)(m - 1)
                                 : (uint32_t)(((uint64_t)i * 0x9E3779B1ull) % (uint64_t)m);
    const uint32_t col = i == 63 ? (uint32_t)(n - 1)
                                 : (uint32_t)(((uint64_t)i * 0x85EBCA6Bull + 7) % (uint64_t)n);
    float got;
    HIP_CHECK(hipMemcpy(&got, static_cast<float*>(g.gold) + (size_t)row * n + col,
                        4, hipMemcpyDeviceToHost));
    const long long want = gemm_host_dot(seed, row, col, k);
    if (got != (float)want) {
      std::printf("gemmtest: gold spot-check FAIL at [%u][%u]: device %.1f, "
                  "host %lld\n", row, col, got, want);
      return 3;
    }
  }
  std::printf("gemmtest: %lldx%lldx%lld, gold by integer VALU in %.1f ms, "
              "spot-check 64/64 vs host%s\n",
              (long long)m, (long long)n, (long long)k, gold_ms,
              inject ? " [fault injection ON]" : "");

  int card = -1;  // sysfs sampling, best effort (as --burn)
  {
    auto topo = k3samd::enumerate_topology(k3samd::default_sysfs_root());
    if (!topo.gpus.empty()) card = topo.gpus[0].card_index;
  }
  if (mem_report_reset(d_report)) return 1;
  const double flops_per = 2.0 * (double)m * (double)n * (double)k;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(now() - t).count();
  };
  std::printf("%6s %10s %12s %6s %7s\n", "t(s)", "iters", "TFLOP/s", "temp",
              "power");
  long max_temp = -1, max_pw = -1;
  long long done = 0, done_last = 0;
  int batch = 1;
  const auto t0 = now();
  auto t_last = t0;
  double next_report = 2.0;
  auto status = [&] {
    auto st = k3samd::read_runtime_stats(k3samd::default_sysfs_root(), card);
    if (st.temp_mc > max_temp) max_temp = st.temp_mc;
    if (st.power_uw > max_pw) max_pw = st.power_uw;
    const double dt = since(t_last);
    std::printf("%6.0f %10lld %12.1f %5ldC %6.0fW\n", since(t0), done,
                dt > 0 ? (done - done_last) * flops_per / dt / 1e12 : 0.0,
                st.temp_mc < 0 ? -1 : st.temp_mc / 1000,
                st.power_uw < 0 ? -1.0 : st.power_uw / 1e6);
    std::fflush(stdout);
    done_last = done;
    t_last = now();
  };
  while (seconds > 0 ? since(t0) < (double)seconds : done < iters) {
    int todo = batch;
    if (seconds <= 0 && todo > iters - done) todo = (int)(iters - done);
    const auto tb = now();
    for (int i = 0; i < todo; ++i) {
      launch_gemm_bf16_nt(0, g.a, g.bt, g.c, g.where, m, n, k);
      if (done == 0 && i == 0 && inject > 0) {
        // operator alerting drill: N single-bit flips at fixed elements of
        // the first result, before its compare
        HIP_CHECK(hipDeviceSynchronize());
        for (int f = 0; f < inject; ++f)
          if (mem_flip(g.c, gemm_inject_elem(f, inject, m, n), 1u << (f % 32)))
            return 1;
      }
      launch_buf_compare(0, g.c, g.gold, m * n / 4, d_report);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    done += todo;
    // size the batch to ~0.2 s between host syncs
    const double per = since(tb) / todo;
    batch = per > 0 ? (int)(0.2 / per) : 64;
    if (batch < 1) batch = 1;
    if (batch > 64) batch = 64;
    if (since(t0) >= next_report) {
      status();
      next_report += 2.0;
    }
  }
  const double total_s = since(t0);
  if (done != done_last) status();  // the tail since the last line

  HostMemReport r;
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  std::vector<int> where((size_t)g.tiles * 2);
  HIP_CHECK(hipMemcpy(where.data(), g.where, where.size() * 4,
                      hipMemcpyDeviceToHost));
  auto xcc_of = [&](unsigned long long elem, unsigned* hw_id) {
    const int64_t row = (int64_t)(elem / (uint64_t)n), col = (int64_t)(elem % (uint64_t)n);
    const int64_t tile = (row / kGemmBM) * (n / kGemmBN) + col / kGemmBN;
    if (hw_id) *hw_id = (unsigned)where[2 * tile + 1];
    return where[2 * tile] & 0xF;
  };
  const bool clean = r.bad_dwords() == 0;
  if (!clean) {
    std::printf("gemmtest: MISCOMPARE - %lld element(s), %lld bit(s)\n",
                r.bad_dwords(), r.bad_bits());
    for (int i = 0; i < r.n_log(); ++i) {
      const long long* rec = r.v + kMemReportHeader + 3 * i;
      unsigned hw_id = 0;
      const int xcc = xcc_of((unsigned long long)rec[0], &hw_id);
      std::printf("C[%llu][%llu] expected 0x%08x actual 0x%08x xor 0x%08x "
                  "xcc %d hw_id 0x%08x\n",
                  (unsigned long long)rec[0] / (unsigned long long)n,
                  (unsigned long long)rec[0] % (unsigned long long)n,
                  (unsigned)rec[1], (unsigned)rec[2],
                  (unsigned)(rec[1] ^ rec[2]), xcc, hw_id);
    }
  }
  std::printf(
      "{\"payload\": \"mi-gemmtest\", \"m\": %lld, \"n\": %lld, \"k\": %lld, "
      "\"iters\": %lld, \"bad_elems\": %lld, \"bad_bits\": %lld, "
      "\"first_bad_row\": %lld, \"first_bad_col\": %lld, "
      "\"first_bad_xcc\": %d, \"avg_tflops\": %.1f, \"gold_ms\": %.1f, "
      "\"max_temp_c\": %ld, \"max_power_w\": %.0f, \"compute_clean\": %s}\n",
      (long long)m, (long long)n, (long long)k, done, r.bad_dwords(),
      r.bad_bits(), clean ? -1LL : (long long)(r.first() / (uint64_t)n),
      clean ? -1LL : (long long)(r.first() % (uint64_t)n),
      clean ? -1 : xcc_of(r.first(), nullptr),
      done * flops_per / total_s / 1e12, gold_ms,
      max_temp < 0 ? -1 : max_temp / 1000, max_pw < 0 ? -1.0 : max_pw / 1e6,
      clean ? "true" : "false");
  if (gemm_free(g)) return 1;
  HIP_CHECK(hipFree(d_report));
  return clean ? 0 : 4;
}

}  // namespace

int main(int argc, char** argv) {
  int64_t mib = 1024;
  int iters = 20;
  int device = 0;
  bool do_mfma = true;
  bool do_check = true;
  bool tune = false;
  bool lds_compare = false;
  bool all_gpus = false;
  int burn_s = 0;
  bool memtest = false;
  int passes = 1, vram_percent = 0, inject = 0;
  bool gemmtest = false;
  int64_t gemm_m = 4096, gemm_n = 4096, gemm_k = 4096;
  int gemm_iters = 0, gemm_seconds = 0, gemm_inject = 0;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--mib") && i + 1 < argc)
      mib = std::atoll(argv[++i]);
    else if (!std::strcmp(argv[i], "--iters") && i + 1 < argc)
      iters = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc)
      device = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--no-mfma"))
      do_mfma = false;
    else if (!std::strcmp(argv[i], "--no-check"))
      do_check = false;
    else if (!std::strcmp(argv[i], "--tune"))
      tune = true;
    else if (!std::strcmp(argv[i], "--lds-compare"))
      lds_compare = true;
    else if (!std::strcmp(argv[i], "--all-gpus"))
      all_gpus = true;
    else if (!std::strcmp(argv[i], "--burn") && i + 1 < argc)
      burn_s = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--memtest"))
      memtest = true;
    else if (!std::strcmp(argv[i], "--passes") && i + 1 < argc)
      passes = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--vram-percent") && i + 1 < argc)
      vram_percent = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--memtest-inject") && i + 1 < argc)
      inject = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--memtest-pattern-dump") && i + 5 < argc)
      return mem_pattern_dump(argv + i + 1);  // host only: before any HIP call
    else if (!std::strcmp(argv[i], "--gemmtest"))
      gemmtest = true;
    else if (!std::strcmp(argv[i], "--gemm-size") && i + 1 < argc)
      gemm_m = gemm_n = gemm_k = std::atoll(argv[++i]);
    else if (!std::strcmp(argv[i], "--gemm-mnk") && i + 3 < argc) {
      gemm_m = std::atoll(argv[++i]);
      gemm_n = std::atoll(argv[++i]);
      gemm_k = std::atoll(argv[++i]);
    } else if (!std::strcmp(argv[i], "--gemm-iters") && i + 1 < argc)
      gemm_iters = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--gemm-seconds") && i + 1 < argc)
      gemm_seconds = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--gemm-inject") && i + 1 < argc)
      gemm_inject = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--gemm-operand-dump") && i + 6 < argc)
      return gemm_operand_dump(argv + i + 1);  // host only: before any HIP call
    else {
      std::printf("mi-stream [--mib N] [--iters N] [--device D] [--no-mfma]"
                  " [--tune] [--lds-compare] [--all-gpus] [--burn SECONDS]"
                  " [--memtest [--passes N] [--vram-percent P]"
                  " [--memtest-inject N]] [--memtest-pattern-dump PATTERN"
                  " SEED INVERT CELL_OFFSET N_CELLS]"
                  " [--gemmtest [--gemm-size S | --gemm-mnk M N K]"
                  " [--gemm-iters I | --gemm-seconds T] [--gemm-inject N]]"
                  " [--gemm-operand-dump WHICH SEED ROW0 COL0 ROWS COLS]\n");
      return !std::strcmp(argv[i], "--help") ? 0 : 2;
    }
  }

  if (memtest &&
      (passes < 1 || mib < 1 || inject < 0 || inject > 16 ||
       (vram_percent != 0 && (vram_percent < 1 || vram_percent > 90)))) {
    std::fprintf(stderr, "mi-stream: --memtest needs --passes >= 1, --mib >= 1,"
                         " --vram-percent 1..90, --memtest-inject 1..16\n");
    return 2;
  }

  if (gemmtest) {
    if (gemm_iters == 0 && gemm_seconds == 0) gemm_seconds = 1;  // default
    if (!k3samd_kern::gemm_shape_ok(gemm_m, gemm_n, gemm_k) ||
        gemm_k > k3samd_kern::kGemmExactMaxK || gemm_iters < 0 ||
        gemm_seconds < 0 || (gemm_iters > 0 && gemm_seconds > 0) ||
        gemm_inject < 0 || gemm_inject > 16) {
      std::fprintf(stderr, "mi-stream: --gemmtest needs M and N multiples of"
                           " 128, K a multiple of 64 and <= 32768, one of"
                           " --gemm-iters >= 1 / --gemm-seconds >= 1,"
                           " --gemm-inject 1..16\n");
      return 2;
    }
  }

  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (ndev == 0) {
    std::fprintf(stderr, "mi-stream: no GPUs visible\n");
    return 1;
  }

  if (all_gpus) {
    if (do_check && !self_check()) return 3;  // oracle on device 0 first
    // concurrent non-temporal triad on every visible GPU (the in-pod
    // demonstration of the headline metric at amd.com/gpu: N): per-GPU
    // buffers + stream, launches overlapped, one global wall-clock.
    const int64_t n_ = mib * (1 << 20) / 4;
    const int64_t n4_ = n_ / 4;
    const double step_bytes = 3.0 * n_ * 4;
    std::vector<f4*> A(ndev), B(ndev), C(ndev);
    std::vector<hipStream_t> streams(ndev);
    for (int d = 0; d < ndev; ++d) {
      HIP_CHECK(hipSetDevice(d));
      HIP_CHECK(hipMalloc(&A[d], n_ * 4));
      HIP_CHECK(hipMalloc(&B[d], n_ * 4));
      HIP_CHECK(hipMalloc(&C[d], n_ * 4));
      HIP_CHECK(hipMemset(B[d], 0x3c, n_ * 4));
      HIP_CHECK(hipMemset(C[d], 0x3d, n_ * 4));
      HIP_CHECK(hipStreamCreate(&streams[d]));
    }
    dim3 g((uint32_t)k3samd_kern::stream_grid(n4_));
    dim3 blk(k3samd_kern::kThreadsPerBlock);
    auto launch_all = [&] {
      for (int d = 0; d < ndev; ++d) {
        (void)hipSetDevice(d);
        k3samd_kern::launch_chunked(n4_, [&](int64_t off, int64_t cnt) {
          dim3 gc((uint32_t)k3samd_kern::stream_grid(cnt));
          hipLaunchKernelGGL(k3samd_kern::stream_triad_kernel<true>, gc, blk,
                             0, streams[d], A[d] + off, B[d] + off,
                             C[d] + off, 2.5f, cnt);
        });
      }
    };
    auto sync_all = [&] {
      for (int d = 0; d < ndev; ++d) (void)hipStreamSynchronize(streams[d]);
    };
    for (int w = 0; w < 3; ++w) launch_all();
    sync_all();
    auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < iters; ++it) launch_all();
    sync_all();
    double sec = std::chrono::duration<double>(
                     std::chrono::steady_clock::now() - t0).count();
    double agg = ndev * step_bytes * iters / sec / 1e9;
    std::printf("mi-stream all-gpus: %d GPU(s) x %lld MiB, aggregate triad "
                "%.1f GB/s (%.1f per GPU)\n",
                ndev, (long long)mib, agg, agg / ndev);
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

  HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));

  const char* gpu_name =
      prop.name[0] ? prop.name : "AMD GPU";  // some boxes report no name
  std::printf("mi-stream: %s (%s), %d visible GPU(s), %d CUs, %.0f GiB VRAM\n",
              gpu_name, prop.gcnArchName, ndev, prop.multiProcessorCount,
              (double)prop.totalGlobalMem / (1 << 30));

  // exit 3: an oracle/self-test failed; exit 4: memtest or gemmtest data
  // miscompare
  if (memtest) return run_memtest(mib, vram_percent, passes, inject, do_check);
  if (gemmtest)
    return run_gemmtest(gemm_m, gemm_n, gemm_k, gemm_iters, gemm_seconds,
                        gemm_inject, do_check);

  if (do_check && !self_check()) return 3;  // pod log is the oracle

  const int64_t n = mib * (1 << 20) / 4;  // fp32 elements
  const int64_t n4 = n / 4;
  const double buf_bytes = (double)n * 4;
  f4 *a, *b, *c;
  HIP_CHECK(hipMalloc(&a, buf_bytes));
  HIP_CHECK(hipMalloc(&b, buf_bytes));
  HIP_CHECK(hipMalloc(&c, buf_bytes));
  HIP_CHECK(hipMemset(b, 0x3c, buf_bytes));
  HIP_CHECK(hipMemset(c, 0x3d, buf_bytes));

  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
  dim3 grid((uint32_t)k3samd_kern::stream_grid(n4));
  dim3 block(k3samd_kern::kThreadsPerBlock);
  const float s = 2.5f;

  if (lds_compare) {
    // direct-nt vs LDS-staged triad (SURVEY §2c blueprint comparison)
    const double bytes = 3 * buf_bytes;
    auto time_k = [&](auto launch_fn) -> double {
      launch_fn();
      (void)hipDeviceSynchronize();
      float best = 1e30f;
      for (int it = 0; it < iters; ++it) {
        (void)hipEventRecord(ev0);
        launch_fn();
        (void)hipEventRecord(ev1);
        (void)hipEventSynchronize(ev1);
        float ms;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        if (ms < best) best = ms;
      }
      return gbps(bytes, best);
    };
    double direct = time_k([&] {
      hipLaunchKernelGGL(k3samd_kern::stream_triad_kernel<true>, grid, block,
                         0, 0, a, b, c, s, n4);
    });
    double lds = time_k([&] {
      hipLaunchKernelGGL(k3samd_kern::stream_triad_lds_kernel, grid, block,
                         0, 0, a, b, c, s, n4);
    });
    std::printf("triad %lld MiB: direct-nt %.1f GB/s | LDS-staged %.1f GB/s "
                "(%.1f%%)\n",
                (long long)mib, direct, lds, 100.0 * lds / direct);
    std::printf("{\"payload\": \"mi-stream-lds\", \"direct_gbps\": %.1f, "
                "\"lds_staged_gbps\": %.1f}\n", direct, lds);
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
    return 0;
  }

  if (tune) {
    // sweep block-size x unroll x grid-occupancy for the grid-stride
    // non-temporal triad; prints GB/s per config (exploration tool)
    const double bytes = 3 * buf_bytes;
    auto time_one = [&](auto kern, int tpb, int blocks) -> double {
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(tpb), 0, 0, a, b, c, s, n4);
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(tpb), 0, 0, a, b, c, s, n4);
      (void)hipDeviceSynchronize();
      float best = 1e30f;
      for (int it = 0; it < iters; ++it) {
        (void)hipEventRecord(ev0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(tpb), 0, 0, a, b, c, s, n4);
        (void)hipEventRecord(ev1);
        (void)hipEventSynchronize(ev1);
        float ms;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        if (ms < best) best = ms;
      }
      return gbps(bytes, best);
    };
    std::printf("tune: grid-stride nt triad, %lld MiB buffers\n",
                (long long)mib);
    std::printf("%8s %6s %8s %10s\n", "tpb", "unroll", "blocks", "GB/s");
    for (int tpb : {256, 512, 1024}) {
      for (int wavesper : {4, 8, 16, 32}) {  // blocks = CUs*waves*64/tpb
        int blocks = 256 * wavesper * 64 / tpb;
        double g1 = time_one(k3samd_kern::stream_triad_gs_kernel<true, 1>,
                             tpb, blocks);
        double g2 = time_one(k3samd_kern::stream_triad_gs_kernel<true, 2>,
                             tpb, blocks);
        double g4 = time_one(k3samd_kern::stream_triad_gs_kernel<true, 4>,
                             tpb, blocks);
        std::printf("%8d %6d %8d  U1 %8.1f U2 %8.1f U4 %8.1f\n", tpb, 1,
                    blocks, g1, g2, g4);
      }
    }
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
    return 0;
  }

  if (burn_s > 0) {
    // Burn-in: saturate HBM (nt triad) and the matrix pipes (bf16 MFMA)
    // concurrently on two streams for --burn seconds, sampling thermals
    // from sysfs. Node-acceptance analog of gpu-burn.
    hipStream_t s_mem, s_mfma;
    HIP_CHECK(hipStreamCreate(&s_mem));
    HIP_CHECK(hipStreamCreate(&s_mfma));
    float* mf_out;
    const int mf_blocks = 1024;
    HIP_CHECK(hipMalloc(&mf_out, mf_blocks * sizeof(float)));
    // resolve our card index for sysfs sampling (best effort)
    int card = -1;
    {
      auto topo = k3samd::enumerate_topology(k3samd::default_sysfs_root());
      if (!topo.gpus.empty()) card = topo.gpus[0].card_index;
    }
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_end = now() + std::chrono::seconds(burn_s);
    // RAS snapshot before the stress: ECC errors that APPEAR during the
    // burn are the node-acceptance failure signal
    k3samd::GpuHealthCounters ras0 =
        k3samd::read_gpu_health(k3samd::default_sysfs_root(), card);
    uint64_t triads = 0, mfmas = 0;
    long max_temp = -1, max_pw = -1;
    std::printf("burn: %d s of concurrent HBM streaming + bf16 MFMA\n",
                burn_s);
    std::printf("%6s %12s %12s %6s %7s %6s\n", "t(s)", "GB/s", "TFLOP/s",
                "temp", "power", "busy");
    auto t0 = now();
    auto next_report = t0 + std::chrono::seconds(2);
    uint64_t triads_last = 0, mfmas_last = 0;
    auto t_last = t0;
    while (now() < t_end) {
      for (int i = 0; i < 8; ++i) {
        hipLaunchKernelGGL(k3samd_kern::stream_triad_kernel<true>, grid,
                           block, 0, s_mem, a, b, c, s, n4);
        hipLaunchKernelGGL(k3samd_kern::mfma_throughput_kernel,
                           dim3(mf_blocks), block, 0, s_mfma, mf_out, 512);
        ++triads;
        ++mfmas;
      }
      HIP_CHECK(hipStreamSynchronize(s_mem));
      HIP_CHECK(hipStreamSynchronize(s_mfma));
      if (now() >= next_report) {
        auto st = k3samd::read_runtime_stats(k3samd::default_sysfs_root(),
                                             card);
        double dt = std::chrono::duration<double>(now() - t_last).count();
        double gbs = (triads - triads_last) * 3.0 * buf_bytes / dt / 1e9;
        double tf =
            (mfmas - mfmas_last) * mf_blocks * 4.0 * 4.0 * 16384.0 * 512.0 /
            dt / 1e12;
        if (st.temp_mc > max_temp) max_temp = st.temp_mc;
        if (st.power_uw > max_pw) max_pw = st.power_uw;
        std::printf("%6.0f %12.1f %12.1f %5ldC %6.0fW %5ld%%\n",
                    std::chrono::duration<double>(now() - t0).count(), gbs,
                    tf, st.temp_mc < 0 ? -1 : st.temp_mc / 1000,
                    st.power_uw < 0 ? -1.0 : st.power_uw / 1e6,
                    st.busy_percent);
        std::fflush(stdout);
        triads_last = triads;
        mfmas_last = mfmas;
        t_last = now();
        next_report += std::chrono::seconds(2);
      }
    }
    double total_s = std::chrono::duration<double>(now() - t0).count();
    double avg_gbs = triads * 3.0 * buf_bytes / total_s / 1e9;
    double avg_tf =
        mfmas * mf_blocks * 4.0 * 4.0 * 16384.0 * 512.0 / total_s / 1e12;
    k3samd::GpuHealthCounters ras1 =
        k3samd::read_gpu_health(k3samd::default_sysfs_root(), card);
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
        total_s, avg_gbs, avg_tf, max_temp < 0 ? -1 : max_temp / 1000,
        max_pw < 0 ? -1.0 : max_pw / 1e6, d_ue, d_ce,
        ras_clean ? "true" : "false");
    HIP_CHECK(hipFree(mf_out));
    HIP_CHECK(hipStreamDestroy(s_mem));
    HIP_CHECK(hipStreamDestroy(s_mfma));
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
    return 0;
  }

  struct Row {
    const char* name;
    double bytes;
    Timing plain, nt;
  };
  Row rows[] = {
      {"copy", 2 * buf_bytes, {}, {}},
      {"scale", 2 * buf_bytes, {}, {}},
      {"add", 3 * buf_bytes, {}, {}},
      {"triad", 3 * buf_bytes, {}, {}},
  };

  auto launch = [&](int op, bool nt) {
    using namespace k3samd_kern;
    // chunked: a flat launch caps at 2^32-1 work-items (AQL grid_size_x),
    // so buffers >= 64 GiB need more than one dispatch
    launch_chunked(n4, [&](int64_t off, int64_t cnt) {
      dim3 g((uint32_t)stream_grid(cnt));
      if (nt) {
        switch (op) {
          case 0: hipLaunchKernelGGL(stream_copy_kernel<true>, g, block, 0, 0, a + off, b + off, cnt); break;
          case 1: hipLaunchKernelGGL(stream_scale_kernel<true>, g, block, 0, 0, a + off, c + off, s, cnt); break;
          case 2: hipLaunchKernelGGL(stream_add_kernel<true>, g, block, 0, 0, a + off, b + off, c + off, cnt); break;
          case 3: hipLaunchKernelGGL(stream_triad_kernel<true>, g, block, 0, 0, a + off, b + off, c + off, s, cnt); break;
        }
      } else {
        switch (op) {
          case 0: hipLaunchKernelGGL(stream_copy_kernel<false>, g, block, 0, 0, a + off, b + off, cnt); break;
          case 1: hipLaunchKernelGGL(stream_scale_kernel<false>, g, block, 0, 0, a + off, c + off, s, cnt); break;
          case 2: hipLaunchKernelGGL(stream_add_kernel<false>, g, block, 0, 0, a + off, b + off, c + off, cnt); break;
          case 3: hipLaunchKernelGGL(stream_triad_kernel<false>, g, block, 0, 0, a + off, b + off, c + off, s, cnt); break;
        }
      }
    });
  };

  for (int op = 0; op < 4; ++op) {
    for (int nt = 0; nt < 2; ++nt) {
      launch(op, nt);  // warm
      launch(op, nt);
      HIP_CHECK(hipDeviceSynchronize());
      Timing& t = nt ? rows[op].nt : rows[op].plain;
      for (int it = 0; it < iters; ++it) {
        HIP_CHECK(hipEventRecord(ev0));
        launch(op, nt);
        HIP_CHECK(hipEventRecord(ev1));
        HIP_CHECK(hipEventSynchronize(ev1));
        float ms;
        HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        if (ms < t.best_ms) t.best_ms = ms;
      }
    }
  }

  std::printf("+--------+-------------------+-------------------+\n");
  std::printf("| STREAM | plain GB/s        | non-temporal GB/s |\n");
  std::printf("+--------+-------------------+-------------------+\n");
  for (auto& r : rows) {
    std::printf("| %-6s | %17.1f | %17.1f |\n", r.name,
                gbps(r.bytes, r.plain.best_ms), gbps(r.bytes, r.nt.best_ms));
  }
  std::printf("+--------+-------------------+-------------------+\n");

  double mfma_tf = 0, mfma32_tf = 0;
  if (do_mfma) {
    // 4096 blocks + 4 chains measured best (tools/mfma_tune.hip sweep:
    // 2477 TF = 99 % of the 2.5 PF dense peak)
    const int blocks = 4096, mf_iters = 4096;
    float* out;
    HIP_CHECK(hipMalloc(&out, blocks * sizeof(float)));
    auto time_mfma = [&](auto kern, double flops_per_wave_iter,
                         int accs) -> double {
      hipLaunchKernelGGL(kern, dim3(blocks), block, 0, 0, out, 256);  // warm
      (void)hipDeviceSynchronize();
      float best = 1e30f;
      for (int rep = 0; rep < 3; ++rep) {  // best-of-3: ride out clock ramp
        (void)hipEventRecord(ev0);
        hipLaunchKernelGGL(kern, dim3(blocks), block, 0, 0, out, mf_iters);
        (void)hipEventRecord(ev1);
        (void)hipEventSynchronize(ev1);
        float ms;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        if (ms < best) best = ms;
      }
      double flops =
          (double)blocks * 4 * accs * flops_per_wave_iter * mf_iters;
      return flops / (best * 1e9);
    };
    mfma_tf = time_mfma(k3samd_kern::mfma_throughput_kernel, 16384.0, 4);
    mfma32_tf = time_mfma(k3samd_kern::mfma_throughput32_kernel, 32768.0, 4);
    double mx8_tf =
        time_mfma(k3samd_kern::mfma_throughput_mx_kernel<0>, 65536.0, 4);
    double mx6_tf =
        time_mfma(k3samd_kern::mfma_throughput_mx_kernel<2>, 65536.0, 4);
    double mx4_tf =
        time_mfma(k3samd_kern::mfma_throughput_mx_kernel<4>, 65536.0, 4);
    std::printf("| MFMA bf16 16x16x32: %7.1f TF | 32x32x16: %7.1f TF     |\n",
                mfma_tf, mfma32_tf);
    std::printf("| MFMA MX 16x16x128  fp8: %6.1f | fp6: %6.1f | fp4: %6.1f |\n",
                mx8_tf, mx6_tf, mx4_tf);
    std::printf("+--------+-------------------+-------------------+\n");
    if (mfma32_tf > mfma_tf) mfma_tf = mfma32_tf;
    HIP_CHECK(hipFree(out));
  }

  double triad_best =
      gbps(rows[3].bytes, std::min(rows[3].plain.best_ms, rows[3].nt.best_ms));
  std::printf(
      "{\"payload\": \"mi-stream\", \"gpu\": \"%s\", \"arch\": \"%s\", "
      "\"buffer_MiB\": %lld, \"triad_gbps\": %.1f, \"mfma_bf16_tflops\": "
      "%.1f}\n",
      gpu_name, prop.gcnArchName, (long long)mib, triad_best, mfma_tf);

  HIP_CHECK(hipFree(a));
  HIP_CHECK(hipFree(b));
  HIP_CHECK(hipFree(c));
  return 0;
}
