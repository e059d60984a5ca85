// mi-mxgemm — verified MX (block-scaled fp8 e4m3 / fp4 e2m1) MFMA GEMM:
// the compute-integrity payload for the instruction class behind the
// MI355X's low-precision peaks (v_mfma_scale_f32_16x16x128_f8f6f4).
//
// The counterpart of `mi-stream --gemmtest` for MX operands: fill A, Bt and
// their E8M0 block scales from mx_pattern.h, compute the product once with
// integer VALU arithmetic (the gold), then loop block-scaled MFMA GEMM ->
// bitwise compare. The operands are chosen so that the fp32 result is exact
// and unique, so any differing bit is a miscompute; each bad element is
// attributed to the XCC / HW_ID of the workgroup that produced it.
//
//   mi-mxgemm [--device D] [--format fp8|fp4] [--size S | --mnk M N K]
//             [--iters I | --seconds T] [--inject N]
//   mi-mxgemm --operand-dump FMT WHICH SEED ROW0 COL0 ROWS COLS
//   mi-mxgemm --scale-dump WHICH SEED ROW0 BLK0 ROWS BLKS
//
// The two dumps are host-only (no HIP call): the raw element codes of a
// logical operand window, and the E8M0 bytes of a window of (stored row,
// k-block). Exit status: 0 clean, 1 HIP error, 2 usage, 3 self-test or
// spot-check failed, 4 data miscompare.
//
// Build: see native/Makefile (links the sysfs topology objects for the
// temperature / power columns).

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../k3samd/ops/hip/mx_gemm_kernels.h"

#define K3_PAYLOAD_NAME "mi-mxgemm"
#include "payload_common.h"

namespace {

using namespace k3samd_kern;

const char kUsage[] =
    "mi-mxgemm [--device D] [--format fp8|fp4] [--size S | --mnk M N K]\n"
    "          [--iters I | --seconds T] [--inject N]\n"
    "mi-mxgemm --operand-dump FMT WHICH SEED ROW0 COL0 ROWS COLS\n"
    "mi-mxgemm --scale-dump WHICH SEED ROW0 BLK0 ROWS BLKS\n";

struct Options {
  int device = 0, fmt = kMxFmtFp8;
  int64_t m = 4096, n = 4096, k = 4096;
  int iters = 0, seconds = 0, inject = 0;
};

const char* fmt_name(int fmt) { return fmt == kMxFmtFp4 ? "fp4" : "fp8"; }

// "fp8" / "fp4" -> the instruction's FMT code, -1 for anything else.
int parse_fmt(const char* s) {
  if (!std::strcmp(s, "fp8")) return kMxFmtFp8;
  if (!std::strcmp(s, "fp4")) return kMxFmtFp4;
  return -1;
}

// Host-side dumps (no HIP call): ROWS lines of COLS integers.
int operand_dump(char** a) {
  const int fmt = parse_fmt(a[0]);
  const int which = std::atoi(a[1]);
  const uint64_t seed = std::strtoull(a[2], nullptr, 0);
  const uint64_t row0 = std::strtoull(a[3], nullptr, 0);
  const uint64_t col0 = std::strtoull(a[4], nullptr, 0);
  const uint64_t rows = std::strtoull(a[5], nullptr, 0);
  const uint64_t cols = std::strtoull(a[6], nullptr, 0);
  if (fmt < 0 || (which != 0 && which != 1)) {
    std::fprintf(stderr, "mi-mxgemm: operand FMT must be fp8 or fp4, WHICH 0 "
                         "(A) or 1 (B)\n");
    return 2;
  }
  for (uint64_t i = 0; i < rows; ++i) {
    for (uint64_t j = 0; j < cols; ++j)
      std::printf("%s%u", j ? " " : "",
                  mx_code(fmt, seed, which, (uint32_t)(row0 + i),
                          (uint32_t)(col0 + j)));
    std::printf("\n");
  }
  return 0;
}

int scale_dump(char** a) {
  const int which = std::atoi(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const uint64_t row0 = std::strtoull(a[2], nullptr, 0);
  const uint64_t blk0 = std::strtoull(a[3], nullptr, 0);
  const uint64_t rows = std::strtoull(a[4], nullptr, 0);
  const uint64_t blks = std::strtoull(a[5], nullptr, 0);
  if (which != 0 && which != 1) {
    std::fprintf(stderr, "mi-mxgemm: scale WHICH must be 0 (SA) or 1 (SB)\n");
    return 2;
  }
  for (uint64_t i = 0; i < rows; ++i) {
    for (uint64_t j = 0; j < blks; ++j)
      std::printf("%s%u", j ? " " : "",
                  (unsigned)mx_scale(seed, which, (uint32_t)(row0 + i),
                                     (uint32_t)(blk0 + j)));
    std::printf("\n");
  }
  return 0;
}

// Host operands of the generator with the block scale applied, in units of
// 1 (fp8) or 1/2 (fp4): a[m * k + kk] and bt[n * k + kk].
void host_operands(int fmt, uint64_t seed, int64_t m, int64_t n, int64_t k,
                   std::vector<int>* a, std::vector<int>* bt) {
  a->resize((size_t)(m * k));
  bt->resize((size_t)(n * k));
  for (int64_t i = 0; i < m; ++i)
    for (int64_t kk = 0; kk < k; ++kk)
      (*a)[i * k + kk] =
          mx_elem_units(fmt, seed, 0, (uint32_t)i, (uint32_t)kk) *
          (1 << (mx_scale(seed, 0, (uint32_t)i, (uint32_t)(kk / 32)) - 127));
  for (int64_t j = 0; j < n; ++j)
    for (int64_t kk = 0; kk < k; ++kk)
      (*bt)[j * k + kk] =
          mx_elem_units(fmt, seed, 1, (uint32_t)kk, (uint32_t)j) *
          (1 << (mx_scale(seed, 1, (uint32_t)j, (uint32_t)(kk / 32)) - 127));
}

// fp32 value of an integer dot product in the format's product units.
float units_to_float(int fmt, long long s) {
  return fmt == kMxFmtFp4 ? (float)s * 0.25f : (float)s;
}

// Element (m, n) of the generator product as a host integer dot product.
long long host_dot(int fmt, uint64_t seed, uint32_t m, uint32_t n, int64_t k) {
  long long s = 0;
  for (int64_t kk = 0; kk < k; ++kk) {
    const uint32_t kb = (uint32_t)(kk / 32);
    const long long a = (long long)mx_elem_units(fmt, seed, 0, m, (uint32_t)kk) *
                        (1 << (mx_scale(seed, 0, m, kb) - 127));
    const long long b = (long long)mx_elem_units(fmt, seed, 1, (uint32_t)kk, n) *
                        (1 << (mx_scale(seed, 1, n, kb) - 127));
    s += a * b;
  }
  return s;
}

// The buffers of one M x N x K problem: packed A[M,K] and Bt[N,K], their
// scales, fp32 C and gold, and the per-tile XCC_ID/HW_ID record.
struct MxBufs {
  DevBuf<void> a, bt, sa, sb;
  DevBuf<float> c, gold;
  DevBuf<int> where;
  int64_t tiles = 0;

  int alloc(int fmt, int64_t m, int64_t n, int64_t k) {
    tiles = (m / kGemmBM) * (n / kGemmBN);
    HIP_CHECK(a.alloc((size_t)(m * mx_row_bytes(fmt, k))));
    HIP_CHECK(bt.alloc((size_t)(n * mx_row_bytes(fmt, k))));
    HIP_CHECK(sa.alloc((size_t)(m * (k / 32))));
    HIP_CHECK(sb.alloc((size_t)(n * (k / 32))));
    HIP_CHECK(c.alloc((size_t)m * n * 4));
    HIP_CHECK(gold.alloc((size_t)m * n * 4));
    HIP_CHECK(where.alloc((size_t)tiles * 8));
    HIP_CHECK(hipMemset(c, 0xFF, (size_t)m * n * 4));  // NaN: unwritten != gold
    HIP_CHECK(hipMemset(where, 0xFF, (size_t)tiles * 8));
    return 0;
  }

  void fill(int fmt, uint64_t seed, int64_t m, int64_t n, int64_t k) {
    launch_mx_fill(0, a, sa, 0, seed, m, k, fmt);
    launch_mx_fill(0, bt, sb, 1, seed, n, k, fmt);
  }
  void gemm(int fmt, int64_t m, int64_t n, int64_t k) {
    launch_mx_gemm_nt(0, fmt, a, sa, bt, sb, c, where, m, n, k);
  }
  void ref(int fmt, int64_t m, int64_t n, int64_t k) {
    launch_mx_gemm_ref_int(0, fmt, a, sa, bt, sb, gold, m, n, k);
  }
};

// Self-test: (1) a 256x256x256 product, the MX MFMA result and (2) the
// integer gold, each against the host integer product of mx_pattern.h;
// (3) the detector drill on C against the gold.
// Returns 0 ok, 3 failed, 1 HIP error.
int selftest(int fmt, void* d_report) {
  const int64_t m = 256, n = 256, k = 256;
  const uint64_t seed = 0x5EEDF00Dull;
  MxBufs g;
  if (g.alloc(fmt, m, n, k)) return 1;
  g.fill(fmt, seed, m, n, k);
  g.ref(fmt, m, n, k);
  g.gemm(fmt, m, n, k);
  HIP_CHECK(hipGetLastError());
  std::vector<float> hc(m * n), hg(m * n);
  HIP_CHECK(hipMemcpy(hc.data(), g.c, hc.size() * 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(hg.data(), g.gold, hg.size() * 4, hipMemcpyDeviceToHost));
  std::vector<int> ha, hbt;
  host_operands(fmt, seed, m, n, k, &ha, &hbt);
  long long bad_mfma = 0, bad_gold = 0;
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < n; ++j) {
      int s = 0;
      for (int64_t kk = 0; kk < k; ++kk) s += ha[i * k + kk] * hbt[j * k + kk];
      const float want = units_to_float(fmt, s);
      if (std::memcmp(&hc[i * n + j], &want, 4)) ++bad_mfma;
      if (std::memcmp(&hg[i * n + j], &want, 4)) ++bad_gold;
    }
  std::printf("mxgemmtest selftest: 256x256x256 %s MX product %s the host "
              "product exactly", fmt_name(fmt),
              bad_mfma ? "DIFFERS from" : "matches");
  if (bad_mfma) std::printf(" (%lld element(s))", bad_mfma);
  std::printf("\nmxgemmtest selftest: integer gold %s the host product exactly",
              bad_gold ? "DIFFERS from" : "matches");
  if (bad_gold) std::printf(" (%lld element(s))", bad_gold);
  std::printf("\n");
  if (bad_mfma || bad_gold) {
    std::printf("mxgemmtest selftest: FAIL\n");
    return 3;
  }

  DrillFlip flips[3] = {{0, 0, 1u << 0},
                        {12345, 0, 1u << 17},
                        {(uint64_t)(m * n - 1), 0, 1u << 31}};
  for (DrillFlip& f : flips) {
    std::memcpy(&f.expect, &hg[f.index], 4);
    if (mem_flip(g.c, f.index, f.mask)) return 1;
  }
  if (mem_report_reset(d_report)) return 1;
  launch_buf_compare(0, g.c, g.gold, m * n / 4, d_report);
  HIP_CHECK(hipGetLastError());
  HostMemReport r;
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  int caught;
  if (!drill_passed(r, flips, &caught)) {
    std::printf("mxgemmtest selftest: FAIL (caught %d/3, bad_elems %lld, "
                "bad_bits %lld, xor_or 0x%08x)\n",
                caught, r.bad_dwords(), r.bad_bits(), r.xor_or());
    return 3;
  }
  std::printf("mxgemmtest selftest: detector caught 3/3 injected flips\n");
  return 0;
}

int run(const Options& o) {
  const int fmt = o.fmt;
  const int64_t m = o.m, n = o.n, k = o.k;
  const uint64_t seed = 0;
  DevBuf<long long> d_report;
  HIP_CHECK(d_report.alloc(sizeof(long long) * kMemReportLen));
  int rc = selftest(fmt, d_report);
  if (rc) return rc;

  MxBufs g;
  if (g.alloc(fmt, m, n, k)) return 1;
  g.fill(fmt, seed, m, n, k);
  float gold_ms;  // one timed launch, no warm-up
  if (EventTimer().best_of(0, 1, [&](bool) { g.ref(fmt, m, n, k); }, &gold_ms))
    return 1;

  // gold spot-check: 64 fixed elements against host integer dot products
  // of the generator — independent of the device entirely
  for (int i = 0; i < 64; ++i) {
    const uint32_t row = i == 63 ? (uint32_t)(m - 1)
                                 : (uint32_t)(((uint64_t)i * 0x9E3779B1ull) % (uint64_t)m);
    const uint32_t col = i == 63 ? (uint32_t)(n - 1)
                                 : (uint32_t)(((uint64_t)i * 0x85EBCA6Bull + 7) % (uint64_t)n);
    float got;
    HIP_CHECK(hipMemcpy(&got, g.gold + (size_t)row * n + col, 4,
                        hipMemcpyDeviceToHost));
    const float want = units_to_float(fmt, host_dot(fmt, seed, row, col, k));
    if (std::memcmp(&got, &want, 4)) {
      std::printf("mxgemmtest: gold spot-check FAIL at [%u][%u]: device %.2f, "
                  "host %.2f\n", row, col, got, want);
      return 3;
    }
  }
  std::printf("mxgemmtest: %s %lldx%lldx%lld, gold by integer VALU in %.1f ms, "
              "spot-check 64/64 vs host%s\n",
              fmt_name(fmt), (long long)m, (long long)n, (long long)k, gold_ms,
              o.inject ? " [fault injection ON]" : "");

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
  while (o.seconds > 0 ? seconds_since(t0) < (double)o.seconds
                       : done < o.iters) {
    int todo = batch;
    if (o.seconds <= 0 && todo > o.iters - done) todo = (int)(o.iters - done);
    const auto tb = Clock::now();
    for (int i = 0; i < todo; ++i) {
      g.gemm(fmt, m, n, k);
      if (done == 0 && i == 0 && o.inject > 0) {
        // operator alerting drill: N single-bit flips (bit f % 32) in the
        // first result before its compare, at elements evenly spaced from 0
        const uint64_t step = (uint64_t)(m * n) / (uint64_t)o.inject;
        HIP_CHECK(hipDeviceSynchronize());
        for (int f = 0; f < o.inject; ++f)
          if (mem_flip(g.c, (uint64_t)f * step, 1u << (f % 32))) return 1;
      }
      launch_buf_compare(0, g.c, g.gold, m * n / 4, d_report);
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
  const double total_s = seconds_since(t0);
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
    std::printf("mxgemmtest: MISCOMPARE - %lld element(s), %lld bit(s)\n",
                r.bad_dwords(), r.bad_bits());
    for (int i = 0; i < r.n_log(); ++i) {
      const long long* rec = r.log(i);
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
      "{\"payload\": \"mi-mxgemmtest\", \"format\": \"%s\", \"m\": %lld, "
      "\"n\": %lld, \"k\": %lld, \"iters\": %lld, \"tflops\": %.1f, "
      "\"compute_clean\": %s, \"bad_elems\": %lld, \"bad_bits\": %lld, "
      "\"first_bad_row\": %lld, \"first_bad_col\": %lld, "
      "\"first_bad_xcc\": %d, \"gold_ms\": %.1f, \"max_temp_c\": %ld, "
      "\"max_power_w\": %.0f}\n",
      fmt_name(fmt), (long long)m, (long long)n, (long long)k, done,
      done * flops_per / total_s / 1e12, clean ? "true" : "false",
      r.bad_dwords(), r.bad_bits(),
      clean ? -1LL : (long long)(r.first() / (uint64_t)n),
      clean ? -1LL : (long long)(r.first() % (uint64_t)n),
      clean ? -1 : xcc_of(r.first(), nullptr), gold_ms, thermal.max_temp_c,
      thermal.max_power_w);
  return clean ? 0 : 4;
}

constexpr int kRun = -1;  // parse_options: no exit status yet, go on

// Flags are matched left to right. The two dump flags run (host only) and
// return as soon as they are reached; an unknown flag, or a flag short of
// its values, prints the usage text and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    auto flag = [&](const char* name, int n_values = 0) {
      return !std::strcmp(argv[i], name) && i + n_values < argc;
    };
    if (flag("--device", 1)) o.device = std::atoi(argv[++i]);
    else if (flag("--format", 1)) o.fmt = parse_fmt(argv[++i]);
    else if (flag("--size", 1)) o.m = o.n = o.k = std::atoll(argv[++i]);
    else if (flag("--mnk", 3)) {
      o.m = std::atoll(argv[++i]);
      o.n = std::atoll(argv[++i]);
      o.k = std::atoll(argv[++i]);
    } else if (flag("--iters", 1)) o.iters = std::atoi(argv[++i]);
    else if (flag("--seconds", 1)) o.seconds = std::atoi(argv[++i]);
    else if (flag("--inject", 1)) {
      o.inject = std::atoi(argv[++i]);
      if (o.inject == 0) o.inject = -1;  // an explicit 0 is out of 1..16
    } else if (flag("--operand-dump", 7)) return operand_dump(argv + i + 1);
    else if (flag("--scale-dump", 6)) return scale_dump(argv + i + 1);
    else {
      std::printf("%s", kUsage);
      return !std::strcmp(argv[i], "--help") ? 0 : 2;
    }
  }
  return kRun;
}

// Range checks before any HIP call. Returns 0 or the exit status 2. Also
// applies the default of one second.
int validate_options(Options& o) {
  if (o.iters == 0 && o.seconds == 0) o.seconds = 1;
  if (!mx_shape_ok(o.fmt, o.m, o.n, o.k) || o.k > kMxExactMaxK ||
      o.iters < 0 || o.seconds < 0 || (o.iters > 0 && o.seconds > 0) ||
      o.inject < 0 || o.inject > 16 || o.device < 0) {
    std::fprintf(stderr, "mi-mxgemm: needs --format fp8 or fp4, M and N "
                         "multiples of 128, K a multiple of 128 (fp8) or 256 "
                         "(fp4) and <= 8192, one of --iters >= 1 / "
                         "--seconds >= 1, --inject 1..16\n");
    return 2;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Options o;
  int rc = parse_options(argc, argv, o);
  if (rc != kRun) return rc;
  if ((rc = validate_options(o)) != 0) return rc;

  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (ndev == 0) {
    std::fprintf(stderr, "mi-mxgemm: no GPUs visible\n");
    return 1;
  }
  hipDeviceProp_t prop;
  HIP_CHECK(hipSetDevice(o.device));
  HIP_CHECK(hipGetDeviceProperties(&prop, o.device));
  std::printf("mi-mxgemm: %s (%s), %d visible GPU(s), %d CUs, MX-%s verified "
              "GEMM\n",
              prop.name[0] ? prop.name : "AMD GPU",  // some boxes report no name
              prop.gcnArchName, ndev, prop.multiProcessorCount,
              fmt_name(o.fmt));
  return run(o);
}
