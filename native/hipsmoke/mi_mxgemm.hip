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
#include "gemm_verify.h"

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

// Generator element (which, row, col) with its block scale applied, in units
// of 1 (fp8) or 1/2 (fp4). The scale belongs to the stored row: m of A, n
// of Bt.
int scaled_units(int fmt, uint64_t seed, int which, uint32_t row, uint32_t col) {
  const uint32_t k = which ? row : col, stored_row = which ? col : row;
  return mx_elem_units(fmt, seed, which, row, col) *
         (1 << (mx_scale(seed, which, stored_row, k / 32) - 127));
}

// fp32 value of an integer dot product in the format's product units.
float units_to_float(int fmt, long long s) {
  return fmt == kMxFmtFp4 ? (float)s * 0.25f : (float)s;
}

// The MX problem of the driver in gemm_verify.h: packed A[M,K] and Bt[N,K]
// of one element format with their E8M0 block scales, from mx_pattern.h.
struct MxProblem {
  using Result = float;
  static constexpr int kPoison = 0xFF;  // NaN
  static constexpr const char* kTag = "mxgemmtest";
  static constexpr int64_t kSelftestK = 256;
  int fmt;
  DevBuf<void> a, bt, sa, sb;
  int64_t m = 0, n = 0, k = 0;

  MxProblem fresh() const { return {fmt}; }
  const char* label() const { return fmt == kMxFmtFp4 ? "fp4 " : "fp8 "; }
  int alloc(int64_t m_, int64_t n_, int64_t k_) {
    m = m_, n = n_, k = k_;
    HIP_CHECK(a.alloc((size_t)(m * mx_row_bytes(fmt, k))));
    HIP_CHECK(bt.alloc((size_t)(n * mx_row_bytes(fmt, k))));
    HIP_CHECK(sa.alloc((size_t)(m * (k / 32))));
    HIP_CHECK(sb.alloc((size_t)(n * (k / 32))));
    return 0;
  }
  void fill(uint64_t seed) {
    launch_mx_fill(0, a, sa, 0, seed, m, k, fmt);
    launch_mx_fill(0, bt, sb, 1, seed, n, k, fmt);
  }
  void gemm(float* c, int* where) {
    launch_mx_gemm_nt(0, fmt, a, sa, bt, sb, c, where, m, n, k);
  }
  void ref(float* gold) {
    launch_mx_gemm_ref_int(0, fmt, a, sa, bt, sb, gold, m, n, k);
  }

  // Element (row, col) of the generator product as a host integer dot product.
  float host_elem(uint64_t seed, uint32_t row, uint32_t col) const {
    long long s = 0;
    for (int64_t kk = 0; kk < k; ++kk)
      s += (long long)scaled_units(fmt, seed, 0, row, (uint32_t)kk) *
           scaled_units(fmt, seed, 1, (uint32_t)kk, col);
    return units_to_float(fmt, s);
  }
  // scaled host operands once (a[m * k + kk], bt[n * k + kk]), then the
  // integer product
  std::vector<float> host_product(uint64_t seed) const {
    std::vector<int> ha(m * k), hbt(n * k);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t kk = 0; kk < k; ++kk)
        ha[i * k + kk] = scaled_units(fmt, seed, 0, (uint32_t)i, (uint32_t)kk);
    for (int64_t j = 0; j < n; ++j)
      for (int64_t kk = 0; kk < k; ++kk)
        hbt[j * k + kk] = scaled_units(fmt, seed, 1, (uint32_t)kk, (uint32_t)j);
    std::vector<float> c(m * n);
    for (int64_t i = 0; i < m; ++i)
      for (int64_t j = 0; j < n; ++j) {
        int s = 0;
        for (int64_t kk = 0; kk < k; ++kk) s += ha[i * k + kk] * hbt[j * k + kk];
        c[i * n + j] = units_to_float(fmt, s);
      }
    return c;
  }
  void print_product_verdict(long long bad_mfma, long long bad_gold) const {
    std::printf("mxgemmtest selftest: 256x256x256 %s MX product %s the host "
                "product exactly", fmt_name(fmt),
                bad_mfma ? "DIFFERS from" : "matches");
    if (bad_mfma) std::printf(" (%lld element(s))", bad_mfma);
    std::printf("\nmxgemmtest selftest: integer gold %s the host product exactly",
                bad_gold ? "DIFFERS from" : "matches");
    if (bad_gold) std::printf(" (%lld element(s))", bad_gold);
    std::printf("\n");
    if (bad_mfma || bad_gold) std::printf("mxgemmtest selftest: FAIL\n");
  }
};

int run(const Options& o) {
  MxProblem p{o.fmt};
  GemmVerifyResult v;
  int rc = gemm_verify(p, o.m, o.n, o.k, o.iters, o.seconds, o.inject, true, &v);
  if (rc) return rc;
  std::printf(
      "{\"payload\": \"mi-mxgemmtest\", \"format\": \"%s\", \"m\": %lld, "
      "\"n\": %lld, \"k\": %lld, \"iters\": %lld, \"tflops\": %.1f, "
      "\"compute_clean\": %s, \"bad_elems\": %lld, \"bad_bits\": %lld, "
      "\"first_bad_row\": %lld, \"first_bad_col\": %lld, "
      "\"first_bad_xcc\": %d, \"gold_ms\": %.1f, \"max_temp_c\": %ld, "
      "\"max_power_w\": %.0f}\n",
      fmt_name(o.fmt), (long long)o.m, (long long)o.n, (long long)o.k, v.iters,
      v.tflops(o.m, o.n, o.k), v.clean() ? "true" : "false",
      v.report.bad_dwords(), v.report.bad_bits(), v.first_bad_row,
      v.first_bad_col, v.first_bad_xcc, v.gold_ms, v.max_temp_c, v.max_power_w);
  return v.clean() ? 0 : 4;
}

// Flags are matched left to right. The two dump flags run (host only) and
// return as soon as they are reached; an unknown flag, or a flag short of
// its values, prints the usage text and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    const FlagMatcher flag{argc, argv, i};
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
    else return usage_status(kUsage, argv[i]);
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
  hipDeviceProp_t prop;
  if (open_device(o.device, &ndev, &prop)) return 1;
  std::printf("mi-mxgemm: %s (%s), %d visible GPU(s), %d CUs, MX-%s verified "
              "GEMM\n",
              prop.name, prop.gcnArchName, ndev, prop.multiProcessorCount,
              fmt_name(o.fmt));
  return run(o);
}
