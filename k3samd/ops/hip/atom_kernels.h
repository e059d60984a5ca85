// Global-atomics integrity test kernels (gfx950), shared by the torch
// extension (k3samd_kernels.hip) and the standalone payload
// (native/hipsmoke/mi_atomtest.hip). Pure HIP, plain C++ and builtins only;
// every atomic is relaxed at agent scope and compiles to its single native
// global_atomic_* instruction (profiles/r12_atomtest.md lists them). No
// kernel here spins or retries: each terminates whatever memory holds.
//
//   atom_fill_kernel     init of every slot, plain stores
//   atom_gold_kernel     one thread per slot folds the W operands in
//                        registers and stores the result: never an atomic,
//                        so it is the independent gold
//   atom_reduce_kernel   W workgroups of 256 lanes; workgroup w walks every
//                        tile of 256 slots and lane l applies operand
//                        (slot = tile * 256 + l, w): each wave-instruction
//                        covers contiguous bytes, every slot receives one
//                        contribution from every workgroup
//   atom_ticket_*        returning fetch-add on C counters, then two plain
//                        kernels that prove every counter's tickets are a
//                        permutation of 0..n-1
//   atom_chain_kernel    swap / compare-and-swap: one launch per round, one
//                        lane per slot, the returned old value is checked
//
// Reports are the memtest's (mem_account, memtest_kernels.h). A dword index
// counts 32-bit words of the tested buffer: slot s of a 4-byte op is dword
// s, of an 8-byte op dwords 2s (low half) and 2s + 1. Final results are
// compared with buf_compare_kernel (gemm_kernels.h).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "atom_pattern.h"
#include "cu_pattern.h"
#include "memtest_kernels.h"

namespace k3samd_kern {

constexpr int kAtomThreads = kAtomTile;
constexpr uint64_t kAtomRotateStep = 40503;  // odd: start tile (w * step) % tiles
constexpr int kAtomMaxChainWgs = 65536;
constexpr int64_t kAtomMaxDraws = 1ll << 30;
constexpr int64_t kAtomMaxCounters = 1ll << 20;
constexpr uint32_t kAtomPermPoison = 0xFFFFFFFFu;

#define K3_ATOM_ORDER __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

using atom_bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using atom_half2 = __attribute__((ext_vector_type(2))) _Float16;

template <typename T>
__device__ __forceinline__ T atom_from_bits(uint64_t bits) {
  T v;
  if constexpr (sizeof(T) == 4) {
    const uint32_t b = (uint32_t)bits;
    __builtin_memcpy(&v, &b, 4);
  } else {
    __builtin_memcpy(&v, &bits, 8);
  }
  return v;
}

template <typename T>
__device__ __forceinline__ uint64_t atom_to_bits(T v) {
  if constexpr (sizeof(T) == 4) {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
  } else {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
  }
}

// The integer ops on the type that selects the instruction.
template <int BASE, typename U, typename S>
__device__ __forceinline__ uint64_t atom_apply_int(void* p, uint64_t bits) {
  U* pu = static_cast<U*>(p);
  S* ps = static_cast<S*>(p);
  const U u = (U)bits;
  const S s = (S)u;
  if constexpr (BASE == kAtomAdd)
    return (uint64_t)__hip_atomic_fetch_add(pu, u, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomAnd)
    return (uint64_t)__hip_atomic_fetch_and(pu, u, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomOr)
    return (uint64_t)__hip_atomic_fetch_or(pu, u, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomXor)
    return (uint64_t)__hip_atomic_fetch_xor(pu, u, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomSmin)
    return (uint64_t)(U)__hip_atomic_fetch_min(ps, s, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomSmax)
    return (uint64_t)(U)__hip_atomic_fetch_max(ps, s, K3_ATOM_ORDER);
  else if constexpr (BASE == kAtomUmin)
    return (uint64_t)__hip_atomic_fetch_min(pu, u, K3_ATOM_ORDER);
  else
    return (uint64_t)__hip_atomic_fetch_max(pu, u, K3_ATOM_ORDER);
}

// One atomic of reduce op OP on the slot at p; returns the old bits. A
// caller that ignores the result gets the no-return instruction.
template <int OP>
__device__ __forceinline__ uint64_t atom_apply(void* p, uint64_t bits) {
  static_assert(OP >= 0 && OP < kAtomReduceOps, "a reduce op");
  if constexpr (OP <= kAtomUmax) {
    return atom_apply_int<OP & 7, uint32_t, int32_t>(p, bits);
  } else if constexpr (OP <= kAtomUmax64) {
    return atom_apply_int<OP & 7, unsigned long long, long long>(p, bits);
  } else if constexpr (OP == kAtomAddF32) {
    return atom_to_bits(__hip_atomic_fetch_add(
        static_cast<float*>(p), atom_from_bits<float>(bits), K3_ATOM_ORDER));
  } else if constexpr (OP == kAtomAddF64) {
    return atom_to_bits(__hip_atomic_fetch_add(
        static_cast<double*>(p), atom_from_bits<double>(bits), K3_ATOM_ORDER));
  } else if constexpr (OP == kAtomMinF64) {
    return atom_to_bits(__hip_atomic_fetch_min(
        static_cast<double*>(p), atom_from_bits<double>(bits), K3_ATOM_ORDER));
  } else if constexpr (OP == kAtomMaxF64) {
    return atom_to_bits(__hip_atomic_fetch_max(
        static_cast<double*>(p), atom_from_bits<double>(bits), K3_ATOM_ORDER));
  } else if constexpr (OP == kAtomPkAddBf16) {
    using V = atom_bf16x2;
    auto* g = (__attribute__((address_space(1))) V*)p;
    return atom_to_bits(__builtin_amdgcn_global_atomic_fadd_v2bf16(
        g, atom_from_bits<V>(bits)));
  } else {
    auto* g = (__attribute__((address_space(1))) atom_half2*)p;
    return atom_to_bits(__builtin_amdgcn_global_atomic_fadd_v2f16(
        g, atom_from_bits<atom_half2>(bits)));
  }
}

// 0 when `old` (a value a returning atomic saw on its way) is compatible
// with the final value of the slot, else the offending bits: the
// order-independent invariants.
//   or   old & ~final == 0      and  final & ~old == 0
//   max  old <= final           min  old >= final      add, xor: none
template <int OP>
__device__ __forceinline__ uint64_t atom_old_violation(uint64_t old,
                                                       uint64_t fin) {
  bool bad = false;
  if constexpr (OP == kAtomMinF64 || OP == kAtomMaxF64) {
    const double o = atom_from_bits<double>(old);
    const double f = atom_from_bits<double>(fin);
    bad = OP == kAtomMinF64 ? !(o >= f) : !(o <= f);
  } else if constexpr (OP > kAtomUmax64) {
    return 0;
  } else {
    constexpr int base = OP & 7;
    constexpr bool wide = OP >= kAtomAdd64;
    if constexpr (base == kAtomOr) return old & ~fin;
    if constexpr (base == kAtomAnd) return fin & ~old;
    if constexpr (base == kAtomUmin) bad = old < fin;
    if constexpr (base == kAtomUmax) bad = old > fin;
    if constexpr (base == kAtomSmin || base == kAtomSmax) {
      const int64_t o = wide ? (int64_t)old : (int64_t)(int32_t)(uint32_t)old;
      const int64_t f = wide ? (int64_t)fin : (int64_t)(int32_t)(uint32_t)fin;
      bad = base == kAtomSmin ? o < f : o > f;
    }
  }
  if (!bad) return 0;
  const uint64_t x = old ^ fin;
  return x != 0 ? x : 1;  // a NaN-free compare cannot fail on equal bits
}

// Fold a slot's difference into the report; EVERY lane of the wave calls
// this (diff = 0 when it has nothing to say). `expect` ^ `diff` is logged as
// the actual value.
__device__ __forceinline__ void atom_account(unsigned long long* report,
                                             bool wide, uint64_t slot,
                                             uint64_t expect, uint64_t diff) {
  u4 e = {0u, 0u, 0u, 0u}, d = {0u, 0u, 0u, 0u};
  uint64_t c;
  if (wide) {
    c = slot >> 1;
    const int k = (int)(slot & 1) * 2;
    e[k] = (uint32_t)expect;
    e[k + 1] = (uint32_t)(expect >> 32);
    d[k] = (uint32_t)diff;
    d[k + 1] = (uint32_t)(diff >> 32);
  } else {
    c = slot >> 2;
    e[(int)(slot & 3)] = (uint32_t)expect;
    d[(int)(slot & 3)] = (uint32_t)diff;
  }
  mem_account(report, c, e, d);
}

__device__ __forceinline__ void atom_store_bits(void* buf, bool wide,
                                                int64_t slot, uint64_t bits) {
  if (wide) static_cast<uint64_t*>(buf)[slot] = bits;
  else static_cast<uint32_t*>(buf)[slot] = (uint32_t)bits;
}

__device__ __forceinline__ uint64_t atom_load_bits(const void* buf, bool wide,
                                                   int64_t slot) {
  return wide ? static_cast<const uint64_t*>(buf)[slot]
              : (uint64_t) static_cast<const uint32_t*>(buf)[slot];
}

__global__ void __launch_bounds__(kAtomThreads)
atom_fill_kernel(void* __restrict__ buf, int64_t slots, int op, uint64_t seed) {
  const int64_t s = (int64_t)blockIdx.x * kAtomThreads + threadIdx.x;
  if (s >= slots) return;  // no cross-lane operation in this kernel
  atom_store_bits(buf, atom_is64(op), s, atom_init(op, seed, (uint64_t)s));
}

__global__ void __launch_bounds__(kAtomThreads)
atom_gold_kernel(void* __restrict__ gold, int64_t slots, int op, uint64_t seed,
                 uint32_t W) {
  const int64_t s = (int64_t)blockIdx.x * kAtomThreads + threadIdx.x;
  if (s >= slots) return;
  atom_store_bits(gold, atom_is64(op), s,
                  atom_expected(op, seed, (uint64_t)s, W));
}

// gridDim.x = W. `drop_w` < 0: no drop. `gold` and `report` are read only
// when RETURNING.
template <int OP, bool RETURNING>
__global__ void __launch_bounds__(kAtomThreads)
atom_reduce_kernel(void* __restrict__ buf, int64_t slots, uint64_t seed,
                   int rotate, int64_t drop_w, int64_t drop_tile,
                   const void* __restrict__ gold,
                   unsigned long long* __restrict__ report) {
  constexpr bool wide = atom_is64(OP);
  const uint32_t w = blockIdx.x, W = gridDim.x;
  const int64_t tiles = (slots + kAtomTile - 1) / kAtomTile;
  const int64_t start =
      rotate ? (int64_t)(((uint64_t)w * kAtomRotateStep) % (uint64_t)tiles) : 0;
  for (int64_t t = 0; t < tiles; ++t) {  // uniform over the grid
    int64_t tile = start + t;
    if (tile >= tiles) tile -= tiles;
    const int64_t s = tile * kAtomTile + threadIdx.x;
    const bool active =
        s < slots && !((int64_t)w == drop_w && tile == drop_tile);
    uint64_t fin = 0, diff = 0;
    if (active) {
      const uint64_t v = atom_operand(OP, seed, (uint64_t)s, w, W);
      void* p = static_cast<char*>(buf) + s * (wide ? 8 : 4);
      if constexpr (RETURNING) {
        const uint64_t old = atom_apply<OP>(p, v);
        fin = atom_load_bits(gold, wide, s);
        diff = atom_old_violation<OP>(old, fin);
      } else {
        (void)atom_apply<OP>(p, v);
      }
    }
    if constexpr (RETURNING)
      atom_account(report, wide, (uint64_t)s, fin, diff);  // all lanes
  }
}

// ---- ticket mode ----

// Thread g draws from counter g % C. T is uint32_t or unsigned long long.
template <typename T>
__global__ void __launch_bounds__(kAtomThreads)
atom_ticket_kernel(T* __restrict__ counters, int64_t C, T* __restrict__ tickets,
                   int64_t n_draws, int* __restrict__ where) {
  const int64_t g = (int64_t)blockIdx.x * kAtomThreads + threadIdx.x;
  if (threadIdx.x == 0) cu_record_placement(where, (int)blockIdx.x);
  if (g >= n_draws) return;
  tickets[g] = __hip_atomic_fetch_add(&counters[g % C], (T)1, K3_ATOM_ORDER);
}

// Draws of counter c among g = 0..n-1 with g % C == c.
__host__ __device__ inline int64_t atom_ticket_draws(int64_t n, int64_t C,
                                                     int64_t c) {
  return c < n ? (n - c + C - 1) / C : 0;
}
// Row length of the perm table: the most draws any counter gets.
__host__ __device__ inline int64_t atom_ticket_row(int64_t n, int64_t C) {
  return (n + C - 1) / C;
}

// perm[c * row + t] = g. A ticket outside its counter's range writes
// nothing (and so leaves an entry unset for the check to find).
template <typename T>
__global__ void __launch_bounds__(kAtomThreads)
atom_ticket_scatter_kernel(const T* __restrict__ tickets, int64_t n_draws,
                           int64_t C, uint32_t* __restrict__ perm) {
  const int64_t g = (int64_t)blockIdx.x * kAtomThreads + threadIdx.x;
  if (g >= n_draws) return;
  const int64_t c = g % C;
  const T t = tickets[g];
  if (t >= (T)atom_ticket_draws(n_draws, C, c)) return;
  perm[c * atom_ticket_row(n_draws, C) + (int64_t)t] = (uint32_t)g;
}

// Entry e < C * row is (c, t) = (e / row, e % row): expected word t, actual
// the ticket of the draw that perm names, all-ones where perm is unset;
// bit 31 of the difference is set when that draw belongs to another counter.
// Padding entries (t >= the counter's draws) must still be unset. Entry
// C * row + c is counter c: expected its draws, actual its final value.
template <typename T>
__global__ void __launch_bounds__(kAtomThreads)
atom_ticket_check_kernel(const T* __restrict__ counters,
                         const T* __restrict__ tickets, int64_t n_draws,
                         int64_t C, const uint32_t* __restrict__ perm,
                         unsigned long long* __restrict__ report) {
  const int64_t e = (int64_t)blockIdx.x * kAtomThreads + threadIdx.x;
  const int64_t row = atom_ticket_row(n_draws, C);
  uint32_t expect = 0, diff = 0;
  if (e < C * row) {
    const int64_t c = e / row, t = e % row;
    const uint32_t g = perm[e];
    if (t >= atom_ticket_draws(n_draws, C, c)) {
      expect = kAtomPermPoison;
      diff = g ^ kAtomPermPoison;
    } else {
      expect = (uint32_t)t;
      if (g == kAtomPermPoison || (int64_t)g >= n_draws) {
        diff = expect ^ kAtomPermPoison;
      } else {
        const T got = tickets[g];
        diff = expect ^ (uint32_t)got;
        if ((uint64_t)got >> 32 != 0 || (int64_t)g % C != c) diff |= 1u << 31;
      }
    }
  } else if (e < C * row + C) {
    const int64_t c = e - C * row;
    const T got = counters[c];
    expect = (uint32_t)atom_ticket_draws(n_draws, C, c);
    diff = expect ^ (uint32_t)got;
    if ((uint64_t)got >> 32 != 0) diff |= 1u << 31;
  }
  atom_account(report, false, (uint64_t)e, expect, diff);  // all lanes
}

// ---- chain mode ----

// Round `round` of a chain op: tile t is served by workgroup
// (t + round) % gridDim.x, so successive rounds reach a slot from different
// workgroups. The slot moves from v_round to v_{round+1}; the returned old
// value must be v_round. cas first tries compare = ~v_round, which must
// fail, return v_round and change nothing.
template <int OP>
__global__ void __launch_bounds__(kAtomThreads)
atom_chain_kernel(void* __restrict__ buf, int64_t slots, uint64_t seed,
                  uint32_t round, unsigned long long* __restrict__ report,
                  int* __restrict__ where) {
  static_assert(OP >= kAtomSwap && OP < kAtomOpCount, "a chain op");
  constexpr bool wide = atom_is64(OP);
  using T = typename std::conditional<wide, unsigned long long, uint32_t>::type;
  if (threadIdx.x == 0) cu_record_placement(where, (int)blockIdx.x);
  const int64_t G = gridDim.x;
  const int64_t tiles = (slots + kAtomTile - 1) / kAtomTile;
  int64_t first = ((int64_t)blockIdx.x - (int64_t)(round % (uint64_t)G)) % G;
  if (first < 0) first += G;
  for (int64_t tile = first; tile < tiles; tile += G) {  // uniform per workgroup
    const int64_t s = tile * kAtomTile + threadIdx.x;
    uint64_t expect = 0, diff = 0;
    if (s < slots) {
      const T cur = (T)atom_chain_value(OP, seed, (uint64_t)s, round);
      const T next = (T)atom_chain_value(OP, seed, (uint64_t)s, (uint64_t)round + 1);
      T* p = static_cast<T*>(buf) + s;
      expect = cur;
      if constexpr (OP == kAtomSwap || OP == kAtomSwap64) {
        diff = (uint64_t)(__hip_atomic_exchange(p, next, K3_ATOM_ORDER) ^ cur);
      } else {
        T seen0 = (T)~cur;  // must fail
        __hip_atomic_compare_exchange_strong(p, &seen0, next, __ATOMIC_RELAXED,
                                             K3_ATOM_ORDER);
        T seen = cur;  // must succeed
        __hip_atomic_compare_exchange_strong(p, &seen, next, __ATOMIC_RELAXED,
                                             K3_ATOM_ORDER);
        diff = (uint64_t)((seen0 ^ cur) | (seen ^ cur));
      }
    }
    atom_account(report, wide, (uint64_t)s, expect, diff);  // all lanes
  }
}

// ---- host-side launchers (no sync, errors via hipGetLastError) ----
// Callers have checked atom_shape_ok(op, slots, W) and the op's mode.

inline uint32_t atom_grid(int64_t n) {
  return (uint32_t)((n + kAtomThreads - 1) / kAtomThreads);
}

inline void launch_atom_fill(hipStream_t stream, void* buf, int64_t slots,
                             int op, uint64_t seed) {
  hipLaunchKernelGGL(atom_fill_kernel, dim3(atom_grid(slots)),
                     dim3(kAtomThreads), 0, stream, buf, slots, op, seed);
}

inline void launch_atom_gold(hipStream_t stream, void* gold, int64_t slots,
                             int op, uint64_t seed, int W) {
  hipLaunchKernelGGL(atom_gold_kernel, dim3(atom_grid(slots)),
                     dim3(kAtomThreads), 0, stream, gold, slots, op, seed,
                     (uint32_t)W);
}

struct AtomReduceArgs {
  void* buf;
  int64_t slots;
  uint64_t seed;
  int W;
  bool rotate = false;
  int64_t drop_w = -1, drop_tile = -1;  // none
  const void* gold = nullptr;           // both set: the returning variant
  void* report = nullptr;
};

template <int OP>
inline void launch_atom_reduce_op(hipStream_t stream, const AtomReduceArgs& a) {
  auto* r = static_cast<unsigned long long*>(a.report);
  if (a.gold != nullptr) {
    hipLaunchKernelGGL((atom_reduce_kernel<OP, true>), dim3((uint32_t)a.W),
                       dim3(kAtomThreads), 0, stream, a.buf, a.slots, a.seed,
                       a.rotate ? 1 : 0, a.drop_w, a.drop_tile, a.gold, r);
  } else {
    hipLaunchKernelGGL((atom_reduce_kernel<OP, false>), dim3((uint32_t)a.W),
                       dim3(kAtomThreads), 0, stream, a.buf, a.slots, a.seed,
                       a.rotate ? 1 : 0, a.drop_w, a.drop_tile, a.gold, r);
  }
}

template <int... OPS>
inline void launch_atom_reduce_table(hipStream_t stream, int op,
                                     const AtomReduceArgs& a,
                                     std::integer_sequence<int, OPS...>) {
  ((op == OPS ? launch_atom_reduce_op<OPS>(stream, a) : (void)0), ...);
}

// `op` is a reduce op (< kAtomReduceOps).
inline void launch_atom_reduce(hipStream_t stream, int op,
                               const AtomReduceArgs& a) {
  launch_atom_reduce_table(stream, op, a,
                           std::make_integer_sequence<int, kAtomReduceOps>{});
}

// counters [C] zeroed by the caller, tickets [n_draws], where
// [atom_grid(n_draws), 2].
inline void launch_atom_ticket(hipStream_t stream, bool wide, void* counters,
                               int64_t C, void* tickets, int64_t n_draws,
                               void* where) {
  const dim3 g(atom_grid(n_draws)), b(kAtomThreads);
  if (wide)
    hipLaunchKernelGGL(atom_ticket_kernel<unsigned long long>, g, b, 0, stream,
                       static_cast<unsigned long long*>(counters), C,
                       static_cast<unsigned long long*>(tickets), n_draws,
                       static_cast<int*>(where));
  else
    hipLaunchKernelGGL(atom_ticket_kernel<uint32_t>, g, b, 0, stream,
                       static_cast<uint32_t*>(counters), C,
                       static_cast<uint32_t*>(tickets), n_draws,
                       static_cast<int*>(where));
}

// Words of the perm table for (n_draws, C).
inline int64_t atom_ticket_perm_words(int64_t n_draws, int64_t C) {
  return C * atom_ticket_row(n_draws, C);
}

// Poisons perm [atom_ticket_perm_words], scatters, checks into `report`.
inline hipError_t launch_atom_ticket_check(hipStream_t stream, bool wide,
                                           const void* counters, int64_t C,
                                           const void* tickets,
                                           int64_t n_draws, void* perm,
                                           void* report) {
  const int64_t words = atom_ticket_perm_words(n_draws, C);
  hipError_t err = hipMemsetAsync(perm, 0xFF, (size_t)words * 4, stream);
  if (err != hipSuccess) return err;
  auto* pm = static_cast<uint32_t*>(perm);
  auto* r = static_cast<unsigned long long*>(report);
  const dim3 gs(atom_grid(n_draws)), gc(atom_grid(words + C)), b(kAtomThreads);
  if (wide) {
    auto* t = static_cast<const unsigned long long*>(tickets);
    auto* c = static_cast<const unsigned long long*>(counters);
    hipLaunchKernelGGL(atom_ticket_scatter_kernel<unsigned long long>, gs, b, 0,
                       stream, t, n_draws, C, pm);
    hipLaunchKernelGGL(atom_ticket_check_kernel<unsigned long long>, gc, b, 0,
                       stream, c, t, n_draws, C, pm, r);
  } else {
    auto* t = static_cast<const uint32_t*>(tickets);
    auto* c = static_cast<const uint32_t*>(counters);
    hipLaunchKernelGGL(atom_ticket_scatter_kernel<uint32_t>, gs, b, 0, stream,
                       t, n_draws, C, pm);
    hipLaunchKernelGGL(atom_ticket_check_kernel<uint32_t>, gc, b, 0, stream, c,
                       t, n_draws, C, pm, r);
  }
  return hipSuccess;
}

// Workgroups of a chain launch over `slots`: one per tile, at most 1024.
inline int atom_chain_wgs(int64_t slots) {
  const int64_t tiles = (slots + kAtomTile - 1) / kAtomTile;
  return (int)(tiles < 1024 ? tiles : 1024);
}

// `op` is a chain op; where [wgs, 2], 1 <= wgs <= kAtomMaxChainWgs.
inline void launch_atom_chain(hipStream_t stream, int op, void* buf,
                              int64_t slots, uint64_t seed, uint32_t round,
                              void* report, void* where, int wgs) {
  auto* r = static_cast<unsigned long long*>(report);
  int* wh = static_cast<int*>(where);
  const dim3 g((uint32_t)wgs), b(kAtomThreads);
  switch (op) {
    case kAtomSwap:
      hipLaunchKernelGGL(atom_chain_kernel<kAtomSwap>, g, b, 0, stream, buf,
                         slots, seed, round, r, wh);
      break;
    case kAtomSwap64:
      hipLaunchKernelGGL(atom_chain_kernel<kAtomSwap64>, g, b, 0, stream, buf,
                         slots, seed, round, r, wh);
      break;
    case kAtomCas:
      hipLaunchKernelGGL(atom_chain_kernel<kAtomCas>, g, b, 0, stream, buf,
                         slots, seed, round, r, wh);
      break;
    default:
      hipLaunchKernelGGL(atom_chain_kernel<kAtomCas64>, g, b, 0, stream, buf,
                         slots, seed, round, r, wh);
      break;
  }
}

}  // namespace k3samd_kern
