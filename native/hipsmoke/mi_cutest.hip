// mi-cutest — per-CU self-test: an LDS march over the whole 160 KiB of every
// compute unit and a VALU signature (fp32 FMA, fp64 FMA, integer multiply /
// dot, cross-lane) on every SIMD, the rung under the GEMM payloads: their
// gold is computed by the integer VALU, and their operands stage through
// the LDS.
//
// Both kernels declare the full LDS, so one workgroup is resident per CU; a
// launch is 4 x CU-count workgroups of either kernel. Every workgroup
// records where it ran, the program keeps launching until every CU (LDS)
// and every SIMD of every CU (VALU) has been seen, and each miscompare is
// printed with its decoded location.
//
//   mi-cutest [--device D] [--seconds S | --iters N] [--passes P]
//             [--rounds R] [--inject N]
//   mi-cutest --signature-dump SEED ROUNDS
//
// The dump is host-only (no HIP call): 64 lines of the four words of a
// lane's signature cell. Exit status: 0 clean, 1 HIP error, 2 usage,
// 3 self-test failed (the tool is broken), 4 miscompare, 5 clean but not
// every CU / SIMD was reached within the launch cap.
//
// Build: see native/Makefile (links the sysfs topology objects for the
// temperature / power columns).

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../k3samd/ops/hip/cu_test_kernels.h"

#define K3_PAYLOAD_NAME "mi-cutest"
#include "payload_common.h"

namespace {

using namespace k3samd_kern;

const char kUsage[] =
    "mi-cutest [--device D] [--seconds S | --iters N] [--passes P]\n"
    "          [--rounds R] [--inject N]\n"
    "mi-cutest --signature-dump SEED ROUNDS\n";

constexpr int kCoverageCap = 8;  // launches granted to reach every CU

struct Options {
  int device = 0, iters = 0, seconds = 0, inject = 0;
  // defaults: ~18 ms of march + ~22 ms of signature per launch on an MI355X
  // (profiles/r07_cutest.md)
  int passes = 256, rounds = 32768;
};

// Host only: the signature of one wave, one lane per line.
int signature_dump(char** a) {
  const uint64_t seed = std::strtoull(a[0], nullptr, 0);
  const long long rounds = std::atoll(a[1]);
  if (rounds < 1 || rounds > (1 << 30)) {
    std::fprintf(stderr, "mi-cutest: signature ROUNDS must be >= 1\n");
    return 2;
  }
  CuSigCell cells[kCuWaveLanes];
  cu_signature_wave(seed, (uint32_t)rounds, cells);
  for (const CuSigCell& c : cells)
    std::printf("0x%08x 0x%08x 0x%08x 0x%08x\n", c.d[0], c.d[1], c.d[2],
                c.d[3]);
  return 0;
}

// Device buffers of one grid: the two placement tables and the expected
// signature.
struct CuBufs {
  int64_t wgs = 0;
  DevBuf<int> lds_where, valu_where;
  DevBuf<void> expected;
  DevBuf<long long> inject;  // up to 16 rows of 5

  int alloc(int64_t n_wgs, uint64_t seed, int rounds,
            std::vector<CuSigCell>* host_expected) {
    wgs = n_wgs;
    HIP_CHECK(lds_where.alloc((size_t)wgs * 8));
    HIP_CHECK(valu_where.alloc((size_t)wgs * kCuWaves * 8));
    HIP_CHECK(expected.alloc(sizeof(CuSigCell) * kCuWaveLanes));
    HIP_CHECK(inject.alloc(sizeof(long long) * 5 * 16));
    host_expected->resize(kCuWaveLanes);
    cu_signature_wave(seed, (uint32_t)rounds, host_expected->data());
    HIP_CHECK(hipMemcpy(expected, host_expected->data(),
                        sizeof(CuSigCell) * kCuWaveLanes,
                        hipMemcpyHostToDevice));
    return 0;
  }
  int clear_where() {
    HIP_CHECK(hipMemset(lds_where, 0xFF, (size_t)wgs * 8));
    HIP_CHECK(hipMemset(valu_where, 0xFF, (size_t)wgs * kCuWaves * 8));
    return 0;
  }
  int set_inject(const std::vector<long long>& rows) {
    HIP_CHECK(hipMemcpy(inject, rows.data(), rows.size() * sizeof(long long),
                        hipMemcpyHostToDevice));
    return 0;
  }
};

// What phase `ph` (0..3) of pass 0 leaves in dword `dw` of workgroup `wg`.
uint32_t lds_expected_dword(uint64_t seed, int64_t wg, int dw, int ph) {
  const int pattern = ph <= 1 ? kMemPatternAddr
                              : ph == 2 ? kMemPatternWalk : kMemPatternChecker;
  return memtest_cell(pattern, seed, ph == 1,
                      (uint64_t)wg * kCuLdsCells + (uint64_t)(dw / 4))
      .d[dw % 4];
}

// Self-test: (1) the device signature of one workgroup against the host
// code of cu_pattern.h; (2) an LDS detector drill and (3) a VALU detector
// drill, three planted flips each. Returns 0 ok, 3 failed, 1 HIP error.
int selftest(void* d_report) {
  const uint64_t seed = 0x5EEDF00Dull;
  const int rounds = 64;
  std::vector<CuSigCell> want;
  CuBufs g;
  if (g.alloc(3, seed, rounds, &want)) return 1;
  HostMemReport r;

  // (1) one workgroup, every wave's cells read back
  DevBuf<void> sig;
  HIP_CHECK(sig.alloc(sizeof(CuSigCell) * kCuWgThreads));
  HIP_CHECK(hipMemset(sig, 0xFF, sizeof(CuSigCell) * kCuWgThreads));
  if (mem_report_reset(d_report) || g.clear_where()) return 1;
  launch_cu_valu_signature(0, d_report, g.valu_where, 1, seed, rounds,
                           g.expected, sig, nullptr, 0);
  HIP_CHECK(hipGetLastError());
  std::vector<CuSigCell> got(kCuWgThreads);
  HIP_CHECK(hipMemcpy(got.data(), sig, sizeof(CuSigCell) * kCuWgThreads,
                      hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(r.v, d_report, sizeof(r.v), hipMemcpyDeviceToHost));
  int bad_cells = 0;
  for (int t = 0; t < kCuWgThreads; ++t)
    if (std::memcmp(&got[t], &want[t & 63], sizeof(CuSigCell))) ++bad_cells;
  std::printf("cutest selftest: device signature of one workgroup (4 waves, "
              "%d rounds) %s the host signature", rounds,
              bad_cells ? "DIFFERS from" : "matches");
  if (bad_cells) std::printf(" (%d cell(s))", bad_cells);
  std::printf("\n");
  if (bad_cells || r.bad_dwords() != 0) {
    std::printf("cutest selftest: FAIL (signature, %lld reported)\n",
                r.bad_dwords());
    return 3;
  }

  // (2) LDS drill on three workgroups: first dword, one inside, last dword
  {
    const long long rows[3][4] = {{0, 0, 1ll << 0, 0},
                                  {1, 12345, 1ll << 17, 1},
                                  {2, kCuLdsDwords - 1, 1ll << 31, 3}};
    DrillFlip flips[3];
    std::vector<long long> flat;
    for (int i = 0; i < 3; ++i) {
      flips[i] = {(uint64_t)rows[i][0] * kCuLdsDwords + (uint64_t)rows[i][1],
                  lds_expected_dword(seed, rows[i][0], (int)rows[i][1],
                                     (int)rows[i][3]),
                  (uint32_t)rows[i][2]};
      flat.insert(flat.end(), rows[i], rows[i] + 4);
    }
    if (g.set_inject(flat) || mem_report_reset(d_report)) return 1;
    launch_cu_lds_march(0, d_report, g.lds_where, 3, seed, 1, 4, g.inject, 3,
                        nullptr);
    HIP_CHECK(hipGetLastError());
    const int rc = drill_verdict(d_report, flips,
                                 {"cutest", "LDS drill ", "bad_dwords",
                                  "LDS detector caught 3/3 planted flips"});
    if (rc) return rc;
  }

  // (3) VALU drill: lane 0 / fp32, a middle lane / fp64 high, lane 63 of
  // wave 3 / integer
  {
    const long long rows[3][5] = {{0, 0, 0, 0, 1ll << 0},
                                  {1, 2, 33, 2, 1ll << 17},
                                  {2, 3, 63, 3, 1ll << 31}};
    DrillFlip flips[3];
    std::vector<long long> flat;
    for (int i = 0; i < 3; ++i) {
      const uint64_t c = (uint64_t)(rows[i][0] * kCuWaves + rows[i][1]) * 64 +
                         (uint64_t)rows[i][2];
      flips[i] = {4 * c + (uint64_t)rows[i][3],
                  want[rows[i][2]].d[rows[i][3]], (uint32_t)rows[i][4]};
      flat.insert(flat.end(), rows[i], rows[i] + 5);
    }
    if (g.set_inject(flat) || mem_report_reset(d_report)) return 1;
    launch_cu_valu_signature(0, d_report, g.valu_where, 3, seed, rounds,
                             g.expected, nullptr, g.inject, 3);
    HIP_CHECK(hipGetLastError());
    return drill_verdict(d_report, flips,
                         {"cutest", "VALU drill ", "bad_dwords",
                          "VALU detector caught 3/3 planted flips"});
  }
}

const char* const kDatapath[5] = {"fp32", "fp64.lo", "fp64.hi", "int",
                                  "lds-fold"};

// Print log records [from, n_log) of one report, decoded against the
// placement tables of the launch that produced them.
void print_miscompares(const HostMemReport& r, int from, bool valu,
                       const std::vector<int>& where) {
  for (int i = from; i < r.n_log(); ++i) {
    const long long* rec = r.log(i);
    const uint64_t g = (uint64_t)rec[0];
    uint64_t wg, row;
    unsigned lane = 0, k = 0, byte = 0;
    if (valu) {
      const uint64_t c = (g >> 2) & (kCuFoldCellBit - 1);
      wg = c / kCuWgThreads;
      row = c / 64;  // wg * 4 + wave
      lane = (unsigned)(c % 64);
      k = ((g >> 2) & kCuFoldCellBit) ? 4u : (unsigned)(g & 3);
    } else {
      wg = row = g / kCuLdsDwords;
      byte = 4u * (unsigned)(g % kCuLdsDwords);
    }
    const unsigned xcc = (unsigned)where[2 * row] & 0xFu;
    const unsigned hw = (unsigned)where[2 * row + 1];
    std::printf("bad %s wg %llu xcc %u se %u sh %u cu %u ", valu ? "valu" : "lds",
                (unsigned long long)wg, xcc, cu_se(hw), cu_sh(hw), cu_cu(hw));
    if (valu)
      std::printf("simd %u lane %u datapath %s ", cu_simd(hw), lane,
                  kDatapath[k]);
    else  // only the workgroup's first wave is recorded: no SIMD to name
      std::printf("simd - byte 0x%05x ", byte);
    std::printf("expected 0x%08x actual 0x%08x xor 0x%08x\n", (unsigned)rec[1],
                (unsigned)rec[2], (unsigned)(rec[1] ^ rec[2]));
  }
}

int run(const Options& o, int cus) {
  const uint64_t seed = 0;
  DevBuf<long long> d_lds_report, d_valu_report;
  HIP_CHECK(d_lds_report.alloc(sizeof(long long) * kMemReportLen));
  HIP_CHECK(d_valu_report.alloc(sizeof(long long) * kMemReportLen));
  int rc = selftest(d_lds_report);
  if (rc) return rc;

  const int64_t wgs = 4 * (int64_t)cus;
  std::vector<CuSigCell> want;
  CuBufs g;
  if (g.alloc(wgs, seed, o.rounds, &want)) return 1;
  if (mem_report_reset(d_lds_report) || mem_report_reset(d_valu_report))
    return 1;

  // operator alerting drill: N flips in the first launch, even ones in the
  // LDS (bit f % 32, phase f % 4), odd ones in the signature (datapath
  // f % 4), on workgroups evenly spaced from 0
  std::vector<long long> lds_rows, valu_rows;
  for (int f = 0; f < o.inject; ++f) {
    const long long wg = (long long)f * (wgs / o.inject);
    if (f % 2 == 0) {
      const long long row[4] = {wg, (long long)f * (kCuLdsDwords / 16),
                                1ll << (f % 32), f % 4};
      lds_rows.insert(lds_rows.end(), row, row + 4);
    } else {
      const long long row[5] = {wg, f % 4, (f * 7) % 64, f % 4,
                                1ll << (f % 32)};
      valu_rows.insert(valu_rows.end(), row, row + 5);
    }
  }
  DevBuf<long long> d_lds_inject, d_valu_inject;
  if (!lds_rows.empty()) {
    HIP_CHECK(d_lds_inject.alloc(lds_rows.size() * sizeof(long long)));
    HIP_CHECK(hipMemcpy(d_lds_inject, lds_rows.data(),
                        lds_rows.size() * sizeof(long long),
                        hipMemcpyHostToDevice));
  }
  if (!valu_rows.empty()) {
    HIP_CHECK(d_valu_inject.alloc(valu_rows.size() * sizeof(long long)));
    HIP_CHECK(hipMemcpy(d_valu_inject, valu_rows.data(),
                        valu_rows.size() * sizeof(long long),
                        hipMemcpyHostToDevice));
  }

  std::printf("cutest: %lld workgroups per launch (4 x %d CUs), %d LDS "
              "pass(es), %d signature rounds%s\n",
              (long long)wgs, cus, o.passes, o.rounds,
              o.inject ? " [fault injection ON]" : "");
  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
  ThermalSampler thermal;
  std::printf("%6s %10s %12s %6s %7s\n", "t(s)", "launches", "LDS GB/s", "temp",
              "power");
  // one march pass moves 4 writes + 4 reads of every workgroup's LDS
  const double lds_bytes_per = 8.0 * kCuLdsBytes * (double)wgs * o.passes;
  std::set<uint32_t> lds_keys, valu_simds;
  std::vector<int> lds_where((size_t)wgs * 2), valu_where((size_t)wgs * 8);
  HostMemReport lr{}, vr{};
  int lds_logged = 0, valu_logged = 0;
  long long done = 0, done_last = 0;
  double march_ms = 0, march_ms_last = 0;
  const auto t0 = Clock::now();
  double next_report = 2.0;
  auto status = [&] {
    thermal.sample();
    const double ms = march_ms - march_ms_last;
    std::printf("%6.0f %10lld %12.0f %s\n", seconds_since(t0), done,
                ms > 0 ? (done - done_last) * lds_bytes_per / ms / 1e6 : 0.0,
                thermal.cells);
    std::fflush(stdout);
    done_last = done;
    march_ms_last = march_ms;
  };
  auto covered = [&] {
    return (long long)lds_keys.size() == cus &&
           (long long)valu_simds.size() == 4ll * cus;
  };
  auto wanted = [&] {
    return o.seconds > 0 ? seconds_since(t0) < (double)o.seconds
                         : done < o.iters;
  };
  while (wanted() || (!covered() && done < kCoverageCap)) {
    const bool first = done == 0;
    if (g.clear_where()) return 1;
    HIP_CHECK(hipEventRecord(ev0));
    launch_cu_lds_march(0, d_lds_report, g.lds_where, wgs, seed, o.passes, 4,
                        first && !lds_rows.empty() ? (long long*)d_lds_inject
                                                   : nullptr,
                        first ? (int)(lds_rows.size() / 4) : 0, nullptr);
    HIP_CHECK(hipEventRecord(ev1));
    launch_cu_valu_signature(
        0, d_valu_report, g.valu_where, wgs, seed, o.rounds, g.expected,
        nullptr,
        first && !valu_rows.empty() ? (long long*)d_valu_inject : nullptr,
        first ? (int)(valu_rows.size() / 5) : 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float ms;
    HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    march_ms += ms;
    ++done;
    HIP_CHECK(hipMemcpy(lds_where.data(), g.lds_where, lds_where.size() * 4,
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(valu_where.data(), g.valu_where, valu_where.size() * 4,
                        hipMemcpyDeviceToHost));
    for (int64_t w = 0; w < wgs; ++w)
      lds_keys.insert(cu_key((uint32_t)lds_where[2 * w],
                             (uint32_t)lds_where[2 * w + 1]));
    for (int64_t s = 0; s < wgs * kCuWaves; ++s) {
      const uint32_t hw = (uint32_t)valu_where[2 * s + 1];
      valu_simds.insert(cu_key((uint32_t)valu_where[2 * s], hw) << 2 |
                        cu_simd(hw));
    }
    // new log records are decoded against THIS launch's placement
    HIP_CHECK(hipMemcpy(lr.v, d_lds_report, sizeof(lr.v), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(vr.v, d_valu_report, sizeof(vr.v), hipMemcpyDeviceToHost));
    if (lr.n_log() > lds_logged || vr.n_log() > valu_logged) {
      std::printf("cutest: MISCOMPARE in launch %lld\n", done);
      print_miscompares(lr, lds_logged, false, lds_where);
      print_miscompares(vr, valu_logged, true, valu_where);
      lds_logged = lr.n_log();
      valu_logged = vr.n_log();
    }
    if (seconds_since(t0) >= next_report) {
      status();
      next_report += 2.0;
    }
  }
  if (done != done_last) status();  // the tail since the last line
  HIP_CHECK(hipEventDestroy(ev0));
  HIP_CHECK(hipEventDestroy(ev1));

  const bool lds_clean = lr.bad_dwords() == 0;
  const bool valu_clean = vr.bad_dwords() == 0;
  const bool clean = lds_clean && valu_clean;
  if (!clean)
    std::printf("cutest: MISCOMPARE - LDS %lld dword(s) %lld bit(s), VALU %lld "
                "dword(s) %lld bit(s)\n",
                lr.bad_dwords(), lr.bad_bits(), vr.bad_dwords(), vr.bad_bits());
  else if (!covered())
    std::printf("cutest: INCOMPLETE - %zu of %d CUs (LDS) and %zu of %d SIMDs "
                "(VALU) reached in %lld launches; not a pass, and no fault "
                "was seen\n",
                lds_keys.size(), cus, valu_simds.size(), 4 * cus, done);
  std::printf(
      "{\"payload\": \"mi-cutest\", \"cus_total\": %d, \"cus_covered\": %zu, "
      "\"simds_covered\": %zu, \"lds_bytes_per_cu\": %d, \"launches\": %lld, "
      "\"passes\": %d, \"rounds\": %d, \"lds_gbs\": %.0f, "
      "\"lds_clean\": %s, \"valu_clean\": %s, \"cu_clean\": %s, "
      "\"covered\": %s, \"bad_dwords\": %lld, \"lds_bad_dwords\": %lld, "
      "\"lds_bad_bits\": %lld, \"valu_bad_dwords\": %lld, "
      "\"valu_bad_bits\": %lld, \"max_temp_c\": %ld, \"max_power_w\": %.0f}\n",
      cus, lds_keys.size(), valu_simds.size(), kCuLdsBytes, done, o.passes,
      o.rounds, march_ms > 0 ? done * lds_bytes_per / march_ms / 1e6 : 0.0,
      lds_clean ? "true" : "false", valu_clean ? "true" : "false",
      clean ? "true" : "false", covered() ? "true" : "false",
      lr.bad_dwords() + vr.bad_dwords(), lr.bad_dwords(), lr.bad_bits(),
      vr.bad_dwords(), vr.bad_bits(), thermal.max_temp_c, thermal.max_power_w);
  return !clean ? 4 : covered() ? 0 : 5;
}

// Flags are matched left to right. --signature-dump runs (host only) and
// returns as soon as it is reached; an unknown flag, or a flag short of its
// values, prints the usage text and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    const FlagMatcher flag{argc, argv, i};
    if (flag("--device", 1)) o.device = std::atoi(argv[++i]);
    else if (flag("--iters", 1)) o.iters = std::atoi(argv[++i]);
    else if (flag("--seconds", 1)) o.seconds = std::atoi(argv[++i]);
    else if (flag("--passes", 1)) o.passes = std::atoi(argv[++i]);
    else if (flag("--rounds", 1)) o.rounds = std::atoi(argv[++i]);
    else if (flag("--inject", 1)) {
      o.inject = std::atoi(argv[++i]);
      if (o.inject == 0) o.inject = -1;  // an explicit 0 is out of 1..16
    } else if (flag("--signature-dump", 2)) return signature_dump(argv + i + 1);
    else return usage_status(kUsage, argv[i]);
  }
  return kRun;
}

// Range checks before any HIP call. Returns 0 or the exit status 2. Also
// applies the default of one second.
int validate_options(Options& o) {
  if (o.iters == 0 && o.seconds == 0) o.seconds = 1;
  if (o.iters < 0 || o.seconds < 0 || (o.iters > 0 && o.seconds > 0) ||
      o.passes < 1 || o.passes > (1 << 20) || o.rounds < 1 ||
      o.rounds > (1 << 30) || o.inject < 0 || o.inject > 16 || o.device < 0) {
    std::fprintf(stderr, "mi-cutest: needs one of --iters >= 1 / --seconds "
                         ">= 1, --passes 1..2^20, --rounds 1..2^30, "
                         "--inject 1..16\n");
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
  std::printf("mi-cutest: %s (%s), %d visible GPU(s), %d CUs, per-CU LDS march "
              "+ VALU signature\n",
              prop.name, prop.gcnArchName, ndev, prop.multiProcessorCount);
  return run(o, prop.multiProcessorCount);
}
