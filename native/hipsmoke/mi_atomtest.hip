// mi-atomtest — global-atomics integrity test: the read-modify-write path
// that split-K and attention-backward reductions, scatter gradients and
// work-queue heads rely on, and that neither the memtest (plain loads and
// stores) nor any GEMM payload (no atomics) ever exercises. Operands are
// chosen so that the correct result is exact and unique in any arrival
// order (atom_pattern.h), an independent gold is computed without atomics,
// and everything is compared bitwise.
//
//   reduce  every op: fill -> gold -> W workgroups apply their operand to
//           every slot -> bitwise compare. Pass p walks rotated when p is
//           odd and uses the value-returning form (with its invariants
//           checked in-kernel) when p & 2.
//   ticket  returning fetch-add on 1, 64 and 1024 counters (32- and 64-bit),
//           proven a permutation by two plain kernels.
//   chain   swap / swap64 / cas / cas64: two rounds, every returned value
//           checked, cas with a must-fail attempt first.
//
//   mi-atomtest [--device N] [--ops all|LIST] [--slots S] [--contributors W]
//               [--seconds T | --iters I] [--inject N]
//   mi-atomtest --pattern-dump OP SEED W SLOT0 N
//
// LIST is comma-separated op names (atom_pattern.h) and/or "ticket". The
// dump is host-only (no HIP call): N lines
//   slot S init 0x.. expected 0x.. operands 0x.. (W of them)
// One table row is printed per op and pass for the first four passes, then
// for one pass every two seconds, each such pass followed by a status line.
// Exit status: 0 clean, 1 HIP error, 2 usage, 3 self-test failed (the tool
// is broken), 4 miscompare.
//
// Build: see native/Makefile.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../k3samd/ops/hip/atom_kernels.h"
#include "../../k3samd/ops/hip/gemm_kernels.h"

#define K3_PAYLOAD_NAME "mi-atomtest"
#include "payload_common.h"

namespace {

using namespace k3samd_kern;

const char kUsage[] =
    "mi-atomtest [--device N] [--ops all|LIST] [--slots S] [--contributors W]\n"
    "            [--seconds T | --iters I] [--inject N]\n"
    "mi-atomtest --pattern-dump OP SEED W SLOT0 N\n";

constexpr int kTicketOp = kAtomOpCount;  // pseudo-op of --ops: the ticket phase
constexpr int kMaxLines = 16;

struct Options {
  int device = 0, iters = 0, seconds = 0, inject = 0;
  long long slots = 1 << 20, contributors = 64;
  std::vector<int> ops;  // empty: all
  bool bad_ops = false;
};

const char* const kInstruction[kAtomOpCount] = {
    "global_atomic_add",        "global_atomic_and",
    "global_atomic_or",         "global_atomic_xor",
    "global_atomic_smin",       "global_atomic_smax",
    "global_atomic_umin",       "global_atomic_umax",
    "global_atomic_add_x2",     "global_atomic_and_x2",
    "global_atomic_or_x2",      "global_atomic_xor_x2",
    "global_atomic_smin_x2",    "global_atomic_smax_x2",
    "global_atomic_umin_x2",    "global_atomic_umax_x2",
    "global_atomic_add_f32",    "global_atomic_add_f64",
    "global_atomic_min_f64",    "global_atomic_max_f64",
    "global_atomic_pk_add_bf16", "global_atomic_pk_add_f16",
    "global_atomic_swap",       "global_atomic_swap_x2",
    "global_atomic_cmpswap",    "global_atomic_cmpswap_x2"};

int op_by_name(const std::string& name) {
  if (name == "ticket") return kTicketOp;
  for (int op = 0; op < kAtomOpCount; ++op)
    if (name == atom_op_name(op)) return op;
  return -1;
}

// Host only.
int pattern_dump(char** a) {
  const int op = op_by_name(a[0]);
  const uint64_t seed = std::strtoull(a[1], nullptr, 0);
  const long long W = std::atoll(a[2]);
  const uint64_t slot0 = std::strtoull(a[3], nullptr, 0);
  const long long n = std::atoll(a[4]);
  if (op < 0 || op >= kAtomOpCount || !atom_shape_ok(op, 1, W) || n < 1 ||
      n > (1 << 20)) {
    std::fprintf(stderr, "mi-atomtest: pattern dump needs a known OP, W within "
                         "the op's cap and 1 <= N <= 2^20\n");
    return 2;
  }
  for (long long i = 0; i < n; ++i) {
    const uint64_t s = slot0 + (uint64_t)i;
    std::printf("slot %llu init 0x%llx expected 0x%llx operands",
                (unsigned long long)s,
                (unsigned long long)atom_init(op, seed, s),
                (unsigned long long)atom_expected(op, seed, s, (uint32_t)W));
    for (long long w = 0; w < W; ++w)
      std::printf(" 0x%llx", (unsigned long long)atom_operand(
                                 op, seed, s, (uint32_t)w, (uint32_t)W));
    std::printf("\n");
  }
  return 0;
}

int64_t padded_bytes(int op, int64_t slots) {
  return (slots * atom_slot_bytes(op) + 15) / 16 * 16;
}

uint64_t host_bits(const std::vector<char>& h, int op, int64_t s) {
  if (atom_is64(op)) {
    uint64_t v;
    std::memcpy(&v, h.data() + 8 * s, 8);
    return v;
  }
  uint32_t v;
  std::memcpy(&v, h.data() + 4 * s, 4);
  return v;
}

// The device buffers of one problem size, sized for the widest op.
struct AtomBufs {
  int64_t slots = 0;
  DevBuf<void> buf, gold;
  DevBuf<int> where;
  DevBuf<long long> report;
  int chain_wgs = 0;

  int alloc(int64_t n) {
    slots = n;
    chain_wgs = atom_chain_wgs(n);
    const size_t bytes = (size_t)padded_bytes(kAtomAdd64, n);
    HIP_CHECK(buf.alloc(bytes));
    HIP_CHECK(gold.alloc(bytes));
    HIP_CHECK(where.alloc((size_t)std::max<int64_t>(chain_wgs, atom_grid(n)) * 8));
    HIP_CHECK(report.alloc(sizeof(long long) * kMemReportLen));
    HIP_CHECK(hipMemset(buf, 0, bytes));  // the padding compares equal
    HIP_CHECK(hipMemset(gold, 0, bytes));
    return 0;
  }
  // Zero the last cell of both padded regions: what lies past the last
  // slot must compare equal whatever op used the buffers before.
  int prepare(int op) {
    const size_t tail = (size_t)padded_bytes(op, slots) - 16;
    HIP_CHECK(hipMemsetAsync(static_cast<char*>((void*)buf) + tail, 0, 16, 0));
    HIP_CHECK(hipMemsetAsync(static_cast<char*>((void*)gold) + tail, 0, 16, 0));
    return 0;
  }
  // fill, gold and the reduce launch; nothing is compared yet.
  int reduce(int op, uint64_t seed, int W, bool rotate, bool returning,
             int64_t drop_w = -1, int64_t drop_tile = -1) {
    if (prepare(op)) return 1;
    launch_atom_fill(0, buf, slots, op, seed);
    launch_atom_gold(0, gold, slots, op, seed, W);
    AtomReduceArgs a{};
    a.buf = buf;
    a.slots = slots;
    a.seed = seed;
    a.W = W;
    a.rotate = rotate;
    a.drop_w = drop_w;
    a.drop_tile = drop_tile;
    if (returning) {
      a.gold = gold;
      a.report = report;
    }
    launch_atom_reduce(0, op, a);
    HIP_CHECK(hipGetLastError());
    return 0;
  }
  int compare(int op) {
    launch_buf_compare(0, buf, gold, padded_bytes(op, slots) / 16, report);
    HIP_CHECK(hipGetLastError());
    return 0;
  }
  int download(int op, std::vector<char>* out, bool from_gold) const {
    out->resize((size_t)slots * atom_slot_bytes(op));
    HIP_CHECK(hipMemcpy(out->data(), from_gold ? (void*)gold : (void*)buf,
                        out->size(), hipMemcpyDeviceToHost));
    return 0;
  }
};

// One ticket run into g.report (which the caller reset): draws = g.slots.
struct TicketBufs {
  DevBuf<void> counters, tickets, perm;
  int alloc(int64_t draws) {
    HIP_CHECK(counters.alloc(8 * 1024));
    HIP_CHECK(tickets.alloc((size_t)draws * 8));
    HIP_CHECK(perm.alloc((size_t)(draws + 1024) * 4));
    return 0;
  }
};

int ticket_draw(AtomBufs& g, TicketBufs& t, bool wide, int64_t C) {
  HIP_CHECK(hipMemset(t.counters, 0, (size_t)C * 8));
  launch_atom_ticket(0, wide, t.counters, C, t.tickets, g.slots, g.where);
  HIP_CHECK(hipGetLastError());
  return 0;
}

int ticket_check(AtomBufs& g, TicketBufs& t, bool wide, int64_t C) {
  HIP_CHECK(launch_atom_ticket_check(0, wide, t.counters, C, t.tickets, g.slots,
                                     t.perm, g.report));
  HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- self-test ----

// Slots of `got` that differ from the host expectation.
long long host_mismatches(const std::vector<char>& got, int op, uint64_t seed,
                          int64_t slots, int W) {
  long long bad = 0;
  for (int64_t s = 0; s < slots; ++s)
    if (host_bits(got, op, s) != atom_expected(op, seed, (uint64_t)s, (uint32_t)W))
      ++bad;
  return bad;
}

// Returns 0 ok, 3 failed, 1 HIP error.
int selftest() {
  const uint64_t seed = 0x5EEDF00Dull;
  const int64_t slots = 4353;
  const int W = 9;
  AtomBufs g;
  TicketBufs t;
  if (g.alloc(slots) || t.alloc(slots)) return 1;
  HostMemReport r;
  std::vector<char> got;

  // (1) every reduce op against the host code, plain and returning + rotated
  long long bad_ops = 0;
  for (int op = 0; op < kAtomReduceOps; ++op) {
    long long bad = 0;
    for (int variant = 0; variant < 2; ++variant) {
      if (mem_report_reset(g.report) ||
          g.reduce(op, seed, W, variant == 1, variant == 1) || g.compare(op))
        return 1;
      if (g.download(op, &got, false)) return 1;
      bad += host_mismatches(got, op, seed, slots, W);
      if (variant == 0) {
        if (g.download(op, &got, true)) return 1;
        bad += host_mismatches(got, op, seed, slots, W);
      }
      if (mem_report_download(r, g.report)) return 1;
      bad += r.bad_dwords();
    }
    if (bad) {
      std::printf("atomtest selftest: op %s DIFFERS from the host expectation "
                  "(%lld)\n", atom_op_name(op), bad);
      ++bad_ops;
    }
  }
  // the chain ops: three rounds, returned values and final memory
  for (int op = kAtomSwap; op < kAtomOpCount; ++op) {
    if (mem_report_reset(g.report)) return 1;
    launch_atom_fill(0, g.buf, slots, op, seed);
    for (uint32_t round = 0; round < 3; ++round)
      launch_atom_chain(0, op, g.buf, slots, seed, round, g.report, g.where,
                        g.chain_wgs);
    HIP_CHECK(hipGetLastError());
    if (g.download(op, &got, false) || mem_report_download(r, g.report))
      return 1;
    const long long bad = host_mismatches(got, op, seed, slots, 3) + r.bad_dwords();
    if (bad) {
      std::printf("atomtest selftest: op %s DIFFERS from the host expectation "
                  "(%lld)\n", atom_op_name(op), bad);
      ++bad_ops;
    }
  }
  // tickets: 8 counters, both widths
  for (int wide = 0; wide < 2; ++wide) {
    if (mem_report_reset(g.report) || ticket_draw(g, t, wide, 8) ||
        ticket_check(g, t, wide, 8) || mem_report_download(r, g.report))
      return 1;
    if (r.bad_dwords()) {
      std::printf("atomtest selftest: %d-bit tickets are no permutation "
                  "(%lld)\n", wide ? 64 : 32, r.bad_dwords());
      ++bad_ops;
    }
  }
  if (bad_ops) {
    std::printf("atomtest selftest: FAIL (%lld op(s) differ)\n", bad_ops);
    return 3;
  }
  std::printf("atomtest selftest: %d ops at %lld slots x %d contributors match "
              "the host expectation (device result and device gold)\n",
              (int)kAtomOpCount, (long long)slots, W);

  // (2) lost-update drill: contributor 4 skips tile 7. For every op whose
  // non-identity operand always changes the slot (all but min / max) the
  // result must differ exactly there, and hold the fold without w = 4.
  const int64_t drop_w = 4, drop_tile = 7;
  for (int op = 0; op < kAtomReduceOps; ++op) {
    const int base = atom_int_base(op);
    if ((atom_is_int(op) && base >= kAtomSmin) || op == kAtomMinF64 ||
        op == kAtomMaxF64)
      continue;
    if (mem_report_reset(g.report) ||
        g.reduce(op, seed, W, false, false, drop_w, drop_tile) ||
        g.compare(op) || g.download(op, &got, false) ||
        mem_report_download(r, g.report))
      return 1;
    long long wrong = 0, dwords = 0;
    for (int64_t s = 0; s < slots; ++s) {
      const bool dropped =
          s / kAtomTile == drop_tile &&
          !atom_operand_is_identity(
              op, atom_operand(op, seed, (uint64_t)s, (uint32_t)drop_w, W));
      const uint64_t full = atom_expected(op, seed, (uint64_t)s, W);
      const uint64_t want =
          dropped ? atom_expected_without(op, seed, (uint64_t)s, W, drop_w)
                  : full;
      const uint64_t have = host_bits(got, op, s);
      if (have != want || (dropped && have == full)) ++wrong;
      dwords += ((uint32_t)(have ^ full) != 0) + ((have ^ full) >> 32 != 0);
    }
    if (wrong || dwords != r.bad_dwords() || dwords == 0) {
      std::printf("atomtest selftest: FAIL (lost-update drill, op %s: %lld "
                  "slot(s) off, %lld dword(s) differ, %lld reported)\n",
                  atom_op_name(op), wrong, dwords, r.bad_dwords());
      return 3;
    }
  }
  std::printf("atomtest selftest: lost-update drill reported exactly the "
              "dropped tile's non-identity slots for every add / and / or / "
              "xor op\n");

  // (3) detector drill: three flips in the result of `add`
  {
    if (mem_report_reset(g.report) || g.reduce(kAtomAdd, seed, W, false, false))
      return 1;
    const uint64_t at[3] = {0, 2049, (uint64_t)slots - 1};
    const uint32_t mask[3] = {1u << 0, 1u << 17, 1u << 31};
    DrillFlip flips[3];
    for (int i = 0; i < 3; ++i) {
      flips[i] = {at[i], (uint32_t)atom_expected(kAtomAdd, seed, at[i], W),
                  mask[i]};
      if (mem_flip(g.buf, at[i], mask[i])) return 1;
    }
    if (g.compare(kAtomAdd)) return 1;
    return drill_verdict(g.report, flips,
                         {"atomtest", "", "bad_dwords",
                          "detector caught 3/3 planted flips"});
  }
}

// ---- run ----

struct Totals {
  long long bad_dwords = 0, bad_bits = 0, first_slot = -1;
  std::string first_op;
  int lines = 0;
};

// Fold one downloaded report into the totals and print its log. `op` is a
// real op or kTicketOp; `where` (chain / ticket) decodes a placement.
void absorb(Totals& tot, const HostMemReport& r, int op, const char* label,
            const std::vector<int>* where, int64_t round, int chain_wgs,
            int64_t draws, int64_t counters) {
  if (r.bad_dwords() == 0) return;
  const bool wide = op != kTicketOp && atom_is64(op);
  if (tot.bad_dwords == 0) {
    tot.first_op = label;
    tot.first_slot = (long long)(wide ? r.first() / 2 : r.first());
  }
  tot.bad_dwords += r.bad_dwords();
  tot.bad_bits += r.bad_bits();
  for (int i = 0; i < r.n_log() && tot.lines < kMaxLines; ++i, ++tot.lines) {
    const long long* rec = r.log(i);
    const uint64_t g = (uint64_t)rec[0];
    if (op == kTicketOp) {
      const int64_t row = atom_ticket_row(draws, counters);
      if ((int64_t)g < counters * row)
        std::printf("bad %s counter %lld ticket %lld ", label,
                    (long long)((int64_t)g / row), (long long)((int64_t)g % row));
      else
        std::printf("bad %s counter %lld final ", label,
                    (long long)((int64_t)g - counters * row));
    } else {
      std::printf("bad %s slot %llu half %d ", label,
                  (unsigned long long)(wide ? g / 2 : g), wide ? (int)(g & 1) : 0);
    }
    std::printf("expected 0x%08x actual 0x%08x xor 0x%08x", (unsigned)rec[1],
                (unsigned)rec[2], (unsigned)(rec[1] ^ rec[2]));
    if (where != nullptr && op != kTicketOp) {
      const int64_t tile = (int64_t)(wide ? g / 2 : g) / kAtomTile;
      const int64_t wg = (tile + round) % chain_wgs;
      std::printf(" xcc %u hw_id 0x%08x", (unsigned)(*where)[2 * wg] & 0xFu,
                  (unsigned)(*where)[2 * wg + 1]);
    }
    std::printf("\n");
  }
}

int run(const Options& o) {
  int rc = selftest();
  if (rc) return rc;

  std::vector<int> ops = o.ops;
  if (ops.empty())
    for (int op = 0; op <= kTicketOp; ++op) ops.push_back(op);
  const int64_t slots = o.slots;
  AtomBufs g;
  TicketBufs t;
  if (g.alloc(slots) || t.alloc(slots)) return 1;

  std::printf("atomtest: %lld slots x %lld contributors (packed ops: %d), "
              "%zu op(s)%s\n", (long long)slots, o.contributors,
              (int)std::min<long long>(o.contributors, kAtomMaxPacked),
              ops.size(), o.inject ? " [fault injection ON]" : "");
  std::printf("%5s %-10s %-26s %9s %10s %9s\n", "pass", "op", "instruction",
              "ms", "Gatomic/s", "GB/s");
  hipEvent_t ev0, ev1;
  HIP_CHECK(hipEventCreate(&ev0));
  HIP_CHECK(hipEventCreate(&ev1));
  ThermalSampler thermal;
  Totals tot;
  HostMemReport r;
  std::vector<int> where((size_t)std::max<int64_t>(g.chain_wgs, atom_grid(slots)) * 2);
  std::vector<double> atoms(kTicketOp + 1, 0.0), ms_sum(kTicketOp + 1, 0.0);
  long long done = 0;
  const auto t0 = Clock::now();
  double next_report = 2.0;
  bool injected = false;
  auto wanted = [&] {
    return o.seconds > 0 ? seconds_since(t0) < (double)o.seconds
                         : done < o.iters;
  };
  while (wanted()) {
    const uint64_t seed = (uint64_t)done;
    const bool rotate = done & 1, returning = (done & 2) != 0;
    const bool show = done < 4 || seconds_since(t0) >= next_report;
    for (int op : ops) {
      float ms = 0;
      double n_atoms = 0;
      int bytes = 4;
      char label[24];
      if (op == kTicketOp) {
        // 32- and 64-bit counters, one, 64 and 1024 of them
        for (int wide = 0; wide < 2; ++wide)
          for (int64_t C : {1, 64, 1024}) {
            float part;
            if (mem_report_reset(g.report)) return 1;
            HIP_CHECK(hipEventRecord(ev0));
            if (ticket_draw(g, t, wide, C)) return 1;
            HIP_CHECK(hipEventRecord(ev1));
            if (ticket_check(g, t, wide, C) || mem_report_download(r, g.report))
              return 1;
            HIP_CHECK(hipEventElapsedTime(&part, ev0, ev1));
            ms += part;
            n_atoms += (double)slots;
            std::snprintf(label, sizeof(label), "ticket%d/%lld", wide ? 64 : 32,
                          (long long)C);
            absorb(tot, r, op, label, nullptr, 0, 1, slots, C);
          }
        std::snprintf(label, sizeof(label), "ticket");
        bytes = 6;  // half the draws are 4-byte, half 8-byte
      } else if (atom_is_chain(op)) {
        std::snprintf(label, sizeof(label), "%s", atom_op_name(op));
        bytes = atom_slot_bytes(op);
        if (g.prepare(op)) return 1;
        launch_atom_fill(0, g.buf, slots, op, seed);
        for (uint32_t round = 0; round < 2; ++round) {
          float part;
          if (mem_report_reset(g.report)) return 1;
          HIP_CHECK(hipEventRecord(ev0));
          launch_atom_chain(0, op, g.buf, slots, seed, round, g.report, g.where,
                            g.chain_wgs);
          HIP_CHECK(hipEventRecord(ev1));
          HIP_CHECK(hipGetLastError());
          if (mem_report_download(r, g.report)) return 1;
          HIP_CHECK(hipMemcpy(where.data(), g.where, (size_t)g.chain_wgs * 8,
                              hipMemcpyDeviceToHost));
          HIP_CHECK(hipEventElapsedTime(&part, ev0, ev1));
          ms += part;
          // cas issues two atomics per slot and round
          n_atoms += (double)slots * (op >= kAtomCas ? 2 : 1);
          absorb(tot, r, op, label, &where, round, g.chain_wgs, 0, 0);
        }
        launch_atom_gold(0, g.gold, slots, op, seed, 2);
        if (mem_report_reset(g.report) || g.compare(op) ||
            mem_report_download(r, g.report))
          return 1;
        absorb(tot, r, op, label, nullptr, 0, 1, 0, 0);
      } else {
        const int W = (int)std::min<long long>(o.contributors, atom_w_cap(op));
        std::snprintf(label, sizeof(label), "%s", atom_op_name(op));
        bytes = atom_slot_bytes(op);
        if (mem_report_reset(g.report) || g.prepare(op)) return 1;
        launch_atom_fill(0, g.buf, slots, op, seed);
        launch_atom_gold(0, g.gold, slots, op, seed, W);
        AtomReduceArgs a{};
        a.buf = g.buf;
        a.slots = slots;
        a.seed = seed;
        a.W = W;
        a.rotate = rotate;
        if (returning) {
          a.gold = g.gold;
          a.report = g.report;
        }
        HIP_CHECK(hipEventRecord(ev0));
        launch_atom_reduce(0, op, a);
        HIP_CHECK(hipEventRecord(ev1));
        HIP_CHECK(hipGetLastError());
        if (o.inject && !injected) {
          // operator alerting drill: one bit in N evenly spaced slots
          injected = true;
          for (int f = 0; f < o.inject; ++f) {
            const uint64_t s = (uint64_t)f * (uint64_t)(slots / o.inject);
            if (mem_flip(g.buf, atom_is64(op) ? 2 * s : s, 1u << (f % 32)))
              return 1;
          }
        }
        if (g.compare(op) || mem_report_download(r, g.report)) return 1;
        HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
        n_atoms = (double)slots * W;
        absorb(tot, r, op, label, nullptr, 0, 1, 0, 0);
      }
      atoms[op] += n_atoms;
      ms_sum[op] += ms;
      if (show)
        std::printf("%5lld %-10s %-26s %9.3f %10.2f %9.1f\n", done, label,
                    op == kTicketOp ? "global_atomic_add[_x2] rtn"
                                    : kInstruction[op],
                    ms, ms > 0 ? n_atoms / ms / 1e6 : 0.0,
                    ms > 0 ? n_atoms * bytes / ms / 1e6 : 0.0);
    }
    ++done;
    if (show) {
      thermal.sample();
      std::printf("status t %.0f s pass %lld bad_dwords %lld %s\n",
                  seconds_since(t0), done, tot.bad_dwords, thermal.cells);
      std::fflush(stdout);
      while (next_report <= seconds_since(t0)) next_report += 2.0;
    }
  }
  thermal.sample();
  HIP_CHECK(hipEventDestroy(ev0));
  HIP_CHECK(hipEventDestroy(ev1));

  const bool clean = tot.bad_dwords == 0;
  if (!clean)
    std::printf("atomtest: MISCOMPARE - %lld dword(s), %lld bit(s), first in "
                "%s\n", tot.bad_dwords, tot.bad_bits, tot.first_op.c_str());
  std::printf("{\"payload\": \"mi-atomtest\", \"ops\": [");
  for (size_t i = 0; i < ops.size(); ++i)
    std::printf("%s\"%s\"", i ? ", " : "",
                ops[i] == kTicketOp ? "ticket" : atom_op_name(ops[i]));
  std::printf("], \"slots\": %lld, \"contributors\": %lld, \"iters\": %lld, "
              "\"atomics_clean\": %s, \"bad_dwords\": %lld, \"bad_bits\": %lld, "
              "\"first_bad_op\": ",
              (long long)slots, o.contributors, done, clean ? "true" : "false",
              tot.bad_dwords, tot.bad_bits);
  if (clean) std::printf("null");
  else std::printf("\"%s\"", tot.first_op.c_str());
  std::printf(", \"first_bad_slot\": %lld", tot.first_slot);
  for (int op : ops)
    std::printf(", \"%s_gatoms\": %.2f",
                op == kTicketOp ? "ticket" : atom_op_name(op),
                ms_sum[op] > 0 ? atoms[op] / ms_sum[op] / 1e6 : 0.0);
  std::printf(", \"max_temp_c\": %ld, \"max_power_w\": %.0f}\n",
              thermal.max_temp_c, thermal.max_power_w);
  return clean ? 0 : 4;
}

// "all" or a comma-separated list of names; an unknown name marks the
// options bad (refused in validate_options).
void parse_ops(const char* arg, Options& o) {
  o.ops.clear();
  if (!std::strcmp(arg, "all")) return;
  std::string list(arg);
  size_t pos = 0;
  while (pos <= list.size()) {
    const size_t end = std::min(list.find(',', pos), list.size());
    const int op = op_by_name(list.substr(pos, end - pos));
    if (op < 0) o.bad_ops = true;
    else o.ops.push_back(op);
    pos = end + 1;
  }
  if (o.ops.empty()) o.bad_ops = true;
}

// Flags are matched left to right. --pattern-dump runs (host only) and
// returns as soon as it is reached; an unknown flag, or a flag short of its
// values, prints the usage text and returns 2 (--help: 0).
int parse_options(int argc, char** argv, Options& o) {
  for (int i = 1; i < argc; ++i) {
    const FlagMatcher flag{argc, argv, i};
    if (flag("--device", 1)) o.device = std::atoi(argv[++i]);
    else if (flag("--iters", 1)) o.iters = std::atoi(argv[++i]);
    else if (flag("--seconds", 1)) o.seconds = std::atoi(argv[++i]);
    else if (flag("--slots", 1)) o.slots = std::atoll(argv[++i]);
    else if (flag("--contributors", 1)) o.contributors = std::atoll(argv[++i]);
    else if (flag("--ops", 1)) parse_ops(argv[++i], o);
    else if (flag("--inject", 1)) {
      o.inject = std::atoi(argv[++i]);
      if (o.inject == 0) o.inject = -1;  // an explicit 0 is out of 1..16
    } else if (flag("--pattern-dump", 5)) return pattern_dump(argv + i + 1);
    else return usage_status(kUsage, argv[i]);
  }
  return kRun;
}

// Range checks before any HIP call. Returns 0 or the exit status 2. Also
// applies the default of one second.
int validate_options(Options& o) {
  if (o.iters == 0 && o.seconds == 0) o.seconds = 1;
  const bool first_is_reduce =
      o.ops.empty() || (o.ops[0] != kTicketOp && !atom_is_chain(o.ops[0]));
  if (o.iters < 0 || o.seconds < 0 || (o.iters > 0 && o.seconds > 0) ||
      o.bad_ops || !atom_shape_ok(kAtomAdd, o.slots, o.contributors) ||
      o.inject < 0 || o.inject > 16 || o.inject > o.slots ||
      (o.inject > 0 && !first_is_reduce) || o.device < 0) {
    std::fprintf(stderr, "mi-atomtest: needs one of --iters >= 1 / --seconds "
                         ">= 1, --slots 1..2^30, --contributors 1..4096, "
                         "--ops all or known names, --inject 1..16 (at most "
                         "one per slot, first op a reduce op)\n");
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
  std::printf("mi-atomtest: %s (%s), %d visible GPU(s), global atomics "
              "integrity test\n", prop.name, prop.gcnArchName, ndev);
  return run(o);
}
