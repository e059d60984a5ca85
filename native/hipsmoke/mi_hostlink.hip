// mi-hostlink — host-link (PCIe) integrity and bandwidth test: verified
// data across the path every workload's data takes to reach the card (host
// DRAM, root complex and IOMMU, the PCIe link, then the copy engines or the
// shader data path), the one path no on-device test touches.
//
// Phases, each marching the memtest patterns (address-unique, complement,
// walking one, checkerboard) with a seed of its own per pass:
//   pull         kernel reads pinned host memory and verifies it
//   push         kernel fills pinned host memory, the host verifies
//   duplex       one launch doing both on disjoint regions
//   h2d / d2h    hipMemcpyAsync (copy engines), verified outside the timing
//   sdma-duplex  both copies on two streams
//   chase        dependent loads through a table in host memory: ns per hop
//                and (final, xor) against the host's expectation
//
//   mi-hostlink [--device N] [--mib M] [--passes P] [--wgs W]
//               [--chase-hops H] [--inject N] [--require-full-link]
//               [--min-gbps X]
//   mi-hostlink --pattern-dump fill PATTERN SEED INVERT CELL_OFFSET N_CELLS
//   mi-hostlink --pattern-dump chase N SEED HOPS
//   mi-hostlink --link-info [--sysfs-root DIR --bdf B]
//
// The dumps and --link-info are host-only (no HIP call). Exit status:
// 0 clean, 1 HIP error, 2 usage, 3 self-test failed (the tool is broken),
// 4 miscompare or wrong chase result, 6 a requested gate failed
// (--require-full-link on a degraded or unreadable link, --min-gbps above
// the slowest single direction). Neither gate is on by default.
//
// Build: see native/Makefile (links the sysfs topology objects).

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../k3samd/ops/hip/hostlink_kernels.h"
#include "../topology/pcie_link.h"

#define K3_PAYLOAD_NAME "mi-hostlink"
#include "payload_common.h"

namespace {

using namespace k3samd_kern;

const char kUsage[] =
    "mi-hostlink [--device N] [--mib M] [--passes P] [--wgs W]\n"
    "            [--chase-hops H] [--inject N] [--require-full-link]\n"
    "            [--min-gbps X]\n"
    "mi-hostlink --pattern-dump fill PATTERN SEED INVERT CELL_OFFSET N_CELLS\n"
    "mi-hostlink --pattern-dump chase N SEED HOPS\n"
    "mi-hostlink --link-info [--sysfs-root DIR --bdf B]\n";

struct Options {
  int device = 0, passes = 1, inject = 0;
  long long mib = 1024;  // per direction; above the 256 MiB Infinity Cache
  int wgs = kLinkDefaultWgs;
  long long chase_hops = 100000;
  bool require_full_link = false, link_info = false;
  double min_gbps = 0;
  std::string sysfs_root, bdf;
};

constexpr uint32_t kChaseSlots = 1u << 16;  // 4 MiB table

// Owning pinned, coherent host allocation with its device-visible address.
class HostBuf {
 public:
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { (void)hipHostFree(p_); }  // hipHostFree(nullptr) is a no-op
  hipError_t alloc(size_t bytes) {
    hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocCoherent);
    if (e != hipSuccess) return e;
    return hipHostGetDevicePointer(&dev_, p_, 0);
  }
  void* host() const { return p_; }
  void* dev() const { return dev_; }

 private:
  void* p_ = nullptr;
  void* dev_ = nullptr;
};

// ---- host-only modes ----

int pattern_dump_fill(char** a) {
  const int pattern = std::atoi(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const int invert = std::atoi(a[2]);
  const uint64_t cell_offset = std::strtoull(a[3], nullptr, 0);
  const long long n_cells = std::atoll(a[4]);
  if (pattern < 0 || pattern >= kMemPatternCount || n_cells < 1 ||
      n_cells > (1 << 20)) {
    std::fprintf(stderr, "mi-hostlink: dump needs PATTERN 0..2 and N_CELLS "
                         "1..2^20\n");
    return 2;
  }
  std::vector<MemCell> cells((size_t)n_cells);
  host_fill(cells.data(), n_cells, MemSpec{seed, pattern, invert ? 1 : 0},
            cell_offset);
  for (const MemCell& c : cells)
    std::printf("0x%08x 0x%08x 0x%08x 0x%08x\n", c.d[0], c.d[1], c.d[2],
                c.d[3]);
  return 0;
}

// "final xor" on the first line, then next(i) of every slot.
int pattern_dump_chase(char** a) {
  const long long n = std::atoll(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const long long hops = std::atoll(a[2]);
  if (!link_chase_n_ok(n) || n > (1 << 20) || hops < 1 ||
      hops > kLinkChaseMaxHops) {
    std::fprintf(stderr, "mi-hostlink: chase dump needs N a power of two in "
                         "2..2^20 and HOPS 1..2^22\n");
    return 2;
  }
  std::vector<uint32_t> table((size_t)n * kLinkSlotDwords);
  link_chase_fill(table.data(), (uint32_t)n, seed);
  const LinkChaseResult r = link_chase_expected((uint32_t)n, seed, hops);
  std::printf("%u %u\n", r.final_index, r.xor_all);
  for (long long i = 0; i < n; ++i)
    std::printf("%u\n", table[(size_t)i * kLinkSlotDwords]);
  return 0;
}

int link_info(const Options& o) {
  const std::string root =
      o.sysfs_root.empty() ? k3samd::default_sysfs_root() : o.sysfs_root;
  const k3samd::PcieLink l = k3samd::read_pcie_link(root, o.bdf);
  std::printf("{\"bdf\": \"%s\", %s, \"numa_node\": %ld, "
              "\"pcie_replay_count\": %ld}\n",
              o.bdf.c_str(), k3samd::pcie_link_json_members(l).c_str(),
              k3samd::read_pcie_device_long(root, o.bdf, "numa_node", -1),
              k3samd::read_pcie_device_long(root, o.bdf, "pcie_replay_count",
                                            -1));
  return 0;
}

// ---- reports ----

void report_clear(HostMemReport& r) { host_report_reset(r.v); }

// Fold `from` into `into` (the log keeps the first 16 records).
void report_merge(HostMemReport& into, const HostMemReport& from) {
  into.v[0] += from.v[0];
  into.v[1] += from.v[1];
  if (from.first() < into.first()) into.v[2] = from.v[2];
  into.v[3] |= from.v[3];
  for (int s = 0; s < from.n_log() && into.v[4] < kMemLogSlots; ++s)
    std::memcpy(into.v + kMemReportHeader + 3 * into.v[4]++, from.log(s),
                3 * sizeof(long long));
}

// N single-bit flips spread from the first dword of the region to the last.
struct Flip {
  uint64_t g;
  uint32_t mask;
};
std::vector<Flip> spread_flips(int64_t n_cells, int n) {
  std::vector<Flip> flips;
  const uint64_t last = 4ull * (uint64_t)n_cells - 1;
  for (int f = 0; f < n; ++f)
    flips.push_back({n > 1 ? last * (uint64_t)f / (uint64_t)(n - 1) : 0,
                     1u << (f % 32)});
  return flips;
}
void plant(void* host, const std::vector<Flip>& flips) {
  for (const Flip& f : flips) static_cast<uint32_t*>(host)[f.g] ^= f.mask;
}

// ---- self-test ----
// (1) the host verifier is clean on a host fill; (2) pull drill: three
// flips planted in host memory, the device must report exactly those;
// (3) push drill: three flips planted in what the device pushed, the host
// verifier must report exactly those; (4) a 1024-slot chase against the
// host's expectation. Returns 0 ok, 3 failed, 1 HIP error.
int selftest(void* d_report, void* d_chase_out) {
  const int64_t n_cells = 65537;  // 1 MiB + one cell: a partial tile
  const MemSpec spec{0x5EEDF00Dull, kMemPatternAddr, 0};
  HostBuf buf;
  HIP_CHECK(buf.alloc((size_t)n_cells * 16));
  const std::vector<Flip> planted = spread_flips(n_cells, 3);
  DrillFlip flips[3];
  for (int i = 0; i < 3; ++i)
    flips[i] = {planted[i].g,
                memtest_cell(spec, planted[i].g / 4).d[planted[i].g % 4],
                planted[i].mask};
  HostMemReport r;

  host_fill(buf.host(), n_cells, spec, 0);
  report_clear(r);
  host_verify(buf.host(), n_cells, spec, 0, r.v);
  if (r.bad_dwords() != 0) {
    std::printf("hostlink selftest: FAIL (host verifier reports %lld bad "
                "dword(s) on its own fill)\n", r.bad_dwords());
    return 3;
  }
  std::printf("hostlink selftest: host verifier clean on a host fill of %lld "
              "cells\n", (long long)n_cells);

  plant(buf.host(), planted);
  if (mem_report_reset(d_report)) return 1;
  launch_link_pull_verify(0, buf.dev(), n_cells, 0, spec, d_report, 3);
  HIP_CHECK(hipGetLastError());
  int rc = drill_verdict(d_report, flips,
                         {"hostlink", "pull drill ", "bad_dwords",
                          "pull detector caught 3/3 flips planted in host "
                          "memory"});
  if (rc) return rc;

  std::memset(buf.host(), 0xFF, (size_t)n_cells * 16);
  launch_link_push_fill(0, buf.dev(), n_cells, 0, spec, 3);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  plant(buf.host(), planted);
  report_clear(r);
  host_verify(buf.host(), n_cells, spec, 0, r.v);
  rc = drill_verdict(r, flips,
                     {"hostlink", "push drill ", "bad_dwords",
                      "host detector caught 3/3 flips planted in pushed data"});
  if (rc) return rc;

  const uint32_t n = 1024;
  const uint64_t hops = 3 * n + 5;
  HostBuf table;
  HIP_CHECK(table.alloc((size_t)n * kLinkSlotBytes));
  link_chase_fill(table.host(), n, spec.seed);
  launch_link_chase(0, table.dev(), n, hops, d_chase_out);
  HIP_CHECK(hipGetLastError());
  unsigned long long out[kLinkChaseOutLen];
  HIP_CHECK(hipMemcpy(out, d_chase_out, sizeof(out), hipMemcpyDeviceToHost));
  const LinkChaseResult want = link_chase_expected(n, spec.seed, hops);
  if (out[0] != want.final_index || out[1] != want.xor_all || out[2] == 0) {
    std::printf("hostlink selftest: FAIL (chase of %u slots: final %llu xor "
                "0x%llx ticks %llu, expected final %u xor 0x%x)\n",
                n, out[0], out[1], out[2], want.final_index, want.xor_all);
    return 3;
  }
  std::printf("hostlink selftest: %u-slot chase matches the host "
              "expectation\n", n);
  return 0;
}

// ---- the run ----

enum Phase { kPull, kPush, kDuplex, kH2D, kD2H, kSdmaDuplex, kPhases };
const char* const kPhaseName[kPhases] = {"pull", "push",        "duplex",
                                         "h2d",  "d2h",         "sdma-duplex"};
const char* const kPhaseKey[kPhases] = {"pull_gbs", "push_gbs", "duplex_gbs",
                                        "h2d_gbs",  "d2h_gbs",
                                        "sdma_duplex_gbs"};

struct Totals {
  double ms[kPhases] = {};
  double bytes[kPhases] = {};
  HostMemReport report[kPhases];
  int lines_printed = 0;  // miscompare lines so far, 16 at most in a run
  double gbs(int ph) const { return ms[ph] > 0 ? bytes[ph] / ms[ph] / 1e6 : 0; }
};

struct Link {
  HostBuf host_r, host_w, table;
  DevBuf<void> dev_in, dev_out;
  DevBuf<long long> d_report;
  DevBuf<unsigned long long> d_chase_out;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done[2] = {nullptr, nullptr};
  hipStream_t side[2] = {nullptr, nullptr};
  int64_t n_cells = 0;
  size_t nbytes = 0;

  ~Link() {
    for (hipEvent_t e : {ev0, ev1, done[0], done[1]})
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : side)
      if (s) (void)hipStreamDestroy(s);
  }

  int setup(const Options& o) {
    nbytes = (size_t)o.mib << 20;
    n_cells = (int64_t)(nbytes / 16);
    HIP_CHECK(d_report.alloc(sizeof(long long) * kMemReportLen));
    HIP_CHECK(d_chase_out.alloc(sizeof(unsigned long long) * kLinkChaseOutLen));
    HIP_CHECK(hipEventCreate(&ev0));
    HIP_CHECK(hipEventCreate(&ev1));
    for (int s = 0; s < 2; ++s) {
      HIP_CHECK(hipEventCreate(&done[s]));
      HIP_CHECK(hipStreamCreateWithFlags(&side[s], hipStreamNonBlocking));
    }
    return 0;
  }
  int alloc_buffers() {
    HIP_CHECK(host_r.alloc(nbytes));
    HIP_CHECK(host_w.alloc(nbytes));
    HIP_CHECK(dev_in.alloc(nbytes));
    HIP_CHECK(dev_out.alloc(nbytes));
    HIP_CHECK(table.alloc((size_t)kChaseSlots * kLinkSlotBytes));
    return 0;
  }
  // Event-time `launch()` on the null stream; *ms receives the interval.
  template <typename Launch>
  int timed(Launch&& launch, float* ms) {
    HIP_CHECK(hipEventRecord(ev0, 0));
    if (launch()) return 1;
    HIP_CHECK(hipEventRecord(ev1, 0));
    HIP_CHECK(hipEventSynchronize(ev1));
    HIP_CHECK(hipEventElapsedTime(ms, ev0, ev1));
    return 0;
  }
  // Both copies at once on the two side streams, fenced by the null stream
  // on either end so that timed() brackets them.
  int both_copies() {
    for (int s = 0; s < 2; ++s) HIP_CHECK(hipStreamWaitEvent(side[s], ev0, 0));
    HIP_CHECK(hipMemcpyAsync(dev_in, host_r.host(), nbytes,
                             hipMemcpyHostToDevice, side[0]));
    HIP_CHECK(hipMemcpyAsync(host_w.host(), dev_out, nbytes,
                             hipMemcpyDeviceToHost, side[1]));
    for (int s = 0; s < 2; ++s) {
      HIP_CHECK(hipEventRecord(done[s], side[s]));
      HIP_CHECK(hipStreamWaitEvent(0, done[s], 0));
    }
    return 0;
  }
};

// The march of one phase: four specs from one seed.
void march_specs(uint64_t seed, MemSpec (&specs)[4]) {
  specs[0] = {seed, kMemPatternAddr, 0};
  specs[1] = {seed, kMemPatternAddr, 1};
  specs[2] = {seed, kMemPatternWalk, 0};
  specs[3] = {seed, kMemPatternChecker, 0};
}

// One phase of one pass; adds to t.ms / t.bytes / t.report[ph].
int run_phase(Link& L, const Options& o, int ph, int pass, Totals& t) {
  MemSpec specs[4];
  march_specs((uint64_t)(7 * pass + ph), specs);
  HostMemReport host_found;
  report_clear(host_found);
  if (mem_report_reset(L.d_report)) return 1;
  const int64_t n = L.n_cells;
  const int duplex_wgs = std::max(2, std::min(2 * o.wgs, kLinkMaxWgs));
  double ms_sum = 0;
  for (int step = 0; step < 4; ++step) {
    const MemSpec spec = specs[step];
    // the second region of a duplex step: next seed, cells after the first
    const MemSpec other{spec.seed + 1, spec.pattern, spec.invert};
    float ms = 0;
    int rc = 0;
    switch (ph) {
      case kPull:
        host_fill(L.host_r.host(), n, spec, 0);
        if (o.inject && pass == 0 && step == 0)
          plant(L.host_r.host(), spread_flips(n, o.inject));
        rc = L.timed([&] {
          launch_link_pull_verify(0, L.host_r.dev(), n, 0, spec, L.d_report,
                                  o.wgs);
          return 0;
        }, &ms);
        break;
      case kPush:
        rc = L.timed([&] {
          launch_link_push_fill(0, L.host_w.dev(), n, 0, spec, o.wgs);
          return 0;
        }, &ms);
        if (!rc) host_verify(L.host_w.host(), n, spec, 0, host_found.v);
        break;
      case kDuplex:
        host_fill(L.host_r.host(), n, spec, 0);
        rc = L.timed([&] {
          launch_link_duplex(0, LinkRegion{L.host_r.dev(), n, 0, spec},
                             LinkRegion{L.host_w.dev(), n, (uint64_t)n, other},
                             L.d_report, duplex_wgs);
          return 0;
        }, &ms);
        if (!rc)
          host_verify(L.host_w.host(), n, other, (uint64_t)n, host_found.v);
        break;
      case kH2D:
        host_fill(L.host_r.host(), n, spec, 0);
        rc = L.timed([&] {
          HIP_CHECK(hipMemcpyAsync(L.dev_in, L.host_r.host(), L.nbytes,
                                   hipMemcpyHostToDevice, 0));
          return 0;
        }, &ms);
        launch_mem_verify(0, L.dev_in, n, 0, spec, L.d_report);
        break;
      case kD2H:
        launch_mem_fill(0, L.dev_out, n, 0, spec, true);
        rc = L.timed([&] {
          HIP_CHECK(hipMemcpyAsync(L.host_w.host(), L.dev_out, L.nbytes,
                                   hipMemcpyDeviceToHost, 0));
          return 0;
        }, &ms);
        if (!rc) host_verify(L.host_w.host(), n, spec, 0, host_found.v);
        break;
      case kSdmaDuplex:
        host_fill(L.host_r.host(), n, spec, 0);
        launch_mem_fill(0, L.dev_out, n, (uint64_t)n, other, true);
        rc = L.timed([&] { return L.both_copies(); }, &ms);
        launch_mem_verify(0, L.dev_in, n, 0, spec, L.d_report);
        if (!rc)
          host_verify(L.host_w.host(), n, other, (uint64_t)n, host_found.v);
        break;
    }
    if (rc) return 1;
    HIP_CHECK(hipGetLastError());
    ms_sum += ms;
  }
  HIP_CHECK(hipDeviceSynchronize());
  HostMemReport found;
  if (mem_report_download(found, L.d_report)) return 1;
  report_merge(found, host_found);
  const double bytes =
      4.0 * (double)L.nbytes * (ph == kDuplex || ph == kSdmaDuplex ? 2 : 1);
  std::printf("%-12s %5d %10.2f %10.1f %12lld\n", kPhaseName[ph], pass,
              bytes / ms_sum / 1e6, ms_sum, found.bad_dwords());
  std::fflush(stdout);
  t.ms[ph] += ms_sum;
  t.bytes[ph] += bytes;
  const int logged = t.report[ph].n_log();
  report_merge(t.report[ph], found);
  if (found.bad_dwords() != 0)
    std::printf("hostlink: MISCOMPARE in phase %s pass %d\n", kPhaseName[ph],
                pass);
  if (t.report[ph].n_log() > logged && t.lines_printed < kMemLogSlots) {
    std::printf("%18s %10s %10s %10s %s\n", "byte offset", "expected",
                "actual", "xor", "phase");
    for (int i = logged;
         i < t.report[ph].n_log() && t.lines_printed < kMemLogSlots;
         ++i, ++t.lines_printed) {
      const long long* rec = t.report[ph].log(i);
      std::printf("0x%016llx 0x%08x 0x%08x 0x%08x %s\n",
                  (unsigned long long)rec[0] * 4, (unsigned)rec[1],
                  (unsigned)rec[2], (unsigned)(rec[1] ^ rec[2]),
                  kPhaseName[ph]);
    }
  }
  return 0;
}

int run(const Options& o, const std::string& bdf, const k3samd::PcieLink& link,
        long numa_node) {
  const std::string root = k3samd::default_sysfs_root();
  Link L;
  if (L.setup(o)) return 1;
  int rc = selftest(L.d_report, L.d_chase_out);
  if (rc) return rc;
  if (L.alloc_buffers()) return 1;
  const long replay_before =
      k3samd::read_pcie_device_long(root, bdf, "pcie_replay_count", -1);

  std::printf("hostlink: %lld MiB per direction, %d pass(es), %d workgroups "
              "per direction (%lld KiB in flight)%s\n",
              o.mib, o.passes, o.wgs,
              (long long)o.wgs * kLinkThreads * 16 * kLinkUnroll / 1024,
              o.inject ? " [fault injection ON]" : "");
  std::printf("%-12s %5s %10s %10s %12s\n", "phase", "pass", "GB/s", "ms",
              "bad dwords");
  Totals t;
  for (HostMemReport& r : t.report) report_clear(r);
  for (int pass = 0; pass < o.passes; ++pass)
    for (int ph = 0; ph < kPhases; ++ph)
      if (run_phase(L, o, ph, pass, t)) return 1;

  // chase: its own seed, one timed walk
  const uint64_t chase_seed = 7ull * (uint64_t)o.passes;
  link_chase_fill(L.table.host(), kChaseSlots, chase_seed);
  launch_link_chase(0, L.table.dev(), kChaseSlots, (uint64_t)o.chase_hops,
                    L.d_chase_out);
  HIP_CHECK(hipGetLastError());
  unsigned long long out[kLinkChaseOutLen];
  HIP_CHECK(hipMemcpy(out, L.d_chase_out, sizeof(out), hipMemcpyDeviceToHost));
  int clock_khz = 0;
  HIP_CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate,
                                  o.device));
  const LinkChaseResult want =
      link_chase_expected(kChaseSlots, chase_seed, (uint64_t)o.chase_hops);
  const bool chase_ok = out[0] == want.final_index && out[1] == want.xor_all;
  const double chase_ns =
      clock_khz > 0 ? (double)out[2] * 1e6 / clock_khz / (double)o.chase_hops
                    : -1.0;
  std::printf("chase: %lld hops over %u slots, %.0f ns per hop, final %llu "
              "xor 0x%08llx%s\n",
              o.chase_hops, kChaseSlots, chase_ns, out[0], out[1],
              chase_ok ? "" : " - WRONG");
  if (!chase_ok)
    std::printf("hostlink: chase expected final %u xor 0x%08x\n",
                want.final_index, want.xor_all);

  const long replay_after =
      k3samd::read_pcie_device_long(root, bdf, "pcie_replay_count", -1);
  const long replay_delta = replay_before >= 0 && replay_after >= 0
                                ? replay_after - replay_before
                                : -1;

  long long bad_dwords = 0, bad_bits = 0;
  int first_phase = -1;
  for (int ph = 0; ph < kPhases; ++ph) {
    bad_dwords += t.report[ph].bad_dwords();
    bad_bits += t.report[ph].bad_bits();
    if (first_phase < 0 && t.report[ph].bad_dwords()) first_phase = ph;
  }
  const bool clean = bad_dwords == 0 && chase_ok;
  const long long first_bad_byte =
      first_phase < 0 ? -1 : (long long)(t.report[first_phase].first() * 4);
  const char* first_bad_phase =
      first_phase >= 0 ? kPhaseName[first_phase] : chase_ok ? "" : "chase";
  if (bad_dwords)
    std::printf("hostlink: MISCOMPARE - %lld dword(s), %lld bit(s), first in "
                "phase %s\n", bad_dwords, bad_bits, first_bad_phase);

  // the gates: the slowest single direction against --min-gbps
  double slowest = t.gbs(kPull);
  for (int ph : {kPush, kH2D, kD2H}) slowest = std::min(slowest, t.gbs(ph));
  const bool link_gate = o.require_full_link && (!link.known || link.degraded);
  const bool rate_gate = o.min_gbps > 0 && slowest < o.min_gbps;
  if (link_gate)
    std::printf("hostlink: GATE --require-full-link: the link is %s\n",
                link.known ? "degraded" : "not readable from sysfs");
  if (rate_gate)
    std::printf("hostlink: GATE --min-gbps %.1f: slowest direction %.2f "
                "GB/s\n", o.min_gbps, slowest);

  std::printf("{\"payload\": \"mi-hostlink\", \"mib\": %lld, \"passes\": %d, "
              "\"wgs\": %d, \"link_clean\": %s, \"bad_dwords\": %lld, "
              "\"bad_bits\": %lld, \"first_bad_byte\": %lld, "
              "\"first_bad_phase\": \"%s\", ",
              o.mib, o.passes, o.wgs, clean ? "true" : "false", bad_dwords,
              bad_bits, first_bad_byte, first_bad_phase);
  for (int ph = 0; ph < kPhases; ++ph)
    std::printf("\"%s\": %.2f, ", kPhaseKey[ph], t.gbs(ph));
  std::printf("\"chase_ns\": %.0f, \"chase_ok\": %s, %s, "
              "\"pcie_replay_delta\": %ld, \"numa_node\": %ld, "
              "\"gates_passed\": %s}\n",
              chase_ns, chase_ok ? "true" : "false",
              k3samd::pcie_link_json_members(link).c_str(), replay_delta,
              numa_node, link_gate || rate_gate ? "false" : "true");
  return !clean ? 4 : link_gate || rate_gate ? 6 : 0;
}

// Flags are matched left to right. --pattern-dump runs (host only) and
// returns as soon as it is reached; an unknown flag, or a flag short of its
// values, prints the usage text and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    const FlagMatcher flag{argc, argv, i};
    if (flag("--device", 1)) o.device = std::atoi(argv[++i]);
    else if (flag("--mib", 1)) o.mib = std::atoll(argv[++i]);
    else if (flag("--passes", 1)) o.passes = std::atoi(argv[++i]);
    else if (flag("--wgs", 1)) o.wgs = std::atoi(argv[++i]);
    else if (flag("--chase-hops", 1)) o.chase_hops = std::atoll(argv[++i]);
    else if (flag("--inject", 1)) {
      o.inject = std::atoi(argv[++i]);
      if (o.inject == 0) o.inject = -1;  // an explicit 0 is out of 1..16
    } else if (flag("--require-full-link")) o.require_full_link = true;
    else if (flag("--min-gbps", 1)) {
      o.min_gbps = std::atof(argv[++i]);
      if (!(o.min_gbps > 0)) o.min_gbps = -1;  // must be a positive rate
    } else if (flag("--link-info")) o.link_info = true;
    else if (flag("--sysfs-root", 1)) o.sysfs_root = argv[++i];
    else if (flag("--bdf", 1)) o.bdf = argv[++i];
    else if (flag("--pattern-dump", 6) && !std::strcmp(argv[i + 1], "fill"))
      return pattern_dump_fill(argv + i + 2);
    else if (flag("--pattern-dump", 4) && !std::strcmp(argv[i + 1], "chase"))
      return pattern_dump_chase(argv + i + 2);
    else return usage_status(kUsage, argv[i]);
  }
  return kRun;
}

// Range checks before any HIP call. Returns 0 or the exit status 2.
int validate_options(const Options& o) {
  if (o.link_info && o.bdf.empty()) {
    std::fprintf(stderr, "mi-hostlink: --link-info needs --bdf B (and "
                         "optionally --sysfs-root DIR)\n");
    return 2;
  }
  if (!o.link_info && (!o.sysfs_root.empty() || !o.bdf.empty())) {
    std::fprintf(stderr, "mi-hostlink: --sysfs-root and --bdf belong to "
                         "--link-info\n");
    return 2;
  }
  if (o.device < 0 || o.mib < 1 || o.mib > (1 << 16) || o.passes < 1 ||
      o.passes > (1 << 20) || !link_wgs_ok(o.wgs) || o.chase_hops < 1 ||
      o.chase_hops > kLinkChaseMaxHops || o.inject < 0 || o.inject > 16 ||
      o.min_gbps < 0) {
    std::fprintf(stderr, "mi-hostlink: needs --mib 1..65536, --passes >= 1, "
                         "--wgs 1..4096, --chase-hops 1..2^22, --inject "
                         "1..16, --min-gbps > 0\n");
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
  if (o.link_info) return link_info(o);

  int ndev = 0;
  hipDeviceProp_t prop;
  if (open_device(o.device, &ndev, &prop)) return 1;
  char bdf[32] = "";
  HIP_CHECK(hipDeviceGetPCIBusId(bdf, sizeof(bdf), o.device));
  for (char* c = bdf; *c; ++c)  // sysfs names are lower case
    if (*c >= 'A' && *c <= 'F') *c += 'a' - 'A';
  const std::string root = k3samd::default_sysfs_root();
  const k3samd::PcieLink link = k3samd::read_pcie_link(root, bdf);
  const long numa_node =
      k3samd::read_pcie_device_long(root, bdf, "numa_node", -1);
  std::printf("mi-hostlink: %s (%s), device %d of %d, bdf %s, numa node %ld, ",
              prop.name, prop.gcnArchName, o.device, ndev, bdf, numa_node);
  if (link.known)
    std::printf("link Gen%d x%d (%.1f GB/s raw)%s\n", link.gen, link.cur_width,
                link.raw_gbps,
                link.degraded ? " - DEGRADED, below the device's maximum" : "");
  else
    std::printf("link unknown (not readable from sysfs)\n");
  return run(o, bdf, link, numa_node);
}
