// HBM memory-test patterns: the expected content of memory as a pure
// function of position. One source of truth for the device kernels
// (memtest_kernels.h) and for host code (mi-stream's pattern dump and
// detector self-test) — no HIP include, so a plain host compiler can use it.
//
// The unit is the 16-byte CELL (one lane's vector access). `c` is a 64-bit
// cell index = caller's cell_offset + position in the tested region; a cell
// is four dwords d0..d3 and the global dword index is g = 4c + k.
//
//   ADDR    address-unique (catches aliasing / address-line faults):
//             x  = lo32(c) ^ (hi32(c) * 0x9E3779B1) ^ lo32(seed)
//             h  = lowbias32(x)
//             d0 = h            d1 = ~h
//             d2 = rotl(h,13) ^ lo32(c)
//             d3 = rotl(h,7)  ^ hi32(c) ^ hi32(seed)
//           d0,d2 recover lo32(c) and d3 recovers hi32(c), so no two cells
//           in the 64-bit range are equal.
//   WALK    dk = 1 << ((lo32(g) + lo32(seed)) & 31)     (walking one)
//   CHECKER dk = ((c + k + seed) & 1) ? 0x55555555 : 0xAAAAAAAA
//
// `invert` complements every dword. All arithmetic is mod 2^32: a few tens
// of 32-bit VALU ops per cell, no 64-bit multiply (a splitmix64-class hash
// per dword would put a ~6 TB/s streaming kernel near the VALU limit).

#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define K3_MEMTEST_HD __host__ __device__
#else
#define K3_MEMTEST_HD
#endif

namespace k3samd_kern {

enum MemPattern : int {
  kMemPatternAddr = 0,
  kMemPatternWalk = 1,
  kMemPatternChecker = 2,
  kMemPatternCount = 3,
};

struct MemCell {
  uint32_t d[4];
};

// One pattern selection: what a region is expected to hold.
struct MemSpec {
  uint64_t seed;
  int pattern;
  int invert;
};

K3_MEMTEST_HD inline uint32_t memtest_rotl32(uint32_t v, int r) {
  return (v << r) | (v >> (32 - r));
}

K3_MEMTEST_HD inline MemCell memtest_cell(int pattern, uint64_t seed,
                                          bool invert, uint64_t c) {
  const uint32_t c_lo = (uint32_t)c, c_hi = (uint32_t)(c >> 32);
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
  MemCell out;
  if (pattern == kMemPatternAddr) {
    uint32_t h = c_lo ^ (c_hi * 0x9E3779B1u) ^ s_lo;
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    out.d[0] = h;
    out.d[1] = ~h;
    out.d[2] = memtest_rotl32(h, 13) ^ c_lo;
    out.d[3] = memtest_rotl32(h, 7) ^ c_hi ^ s_hi;
  } else if (pattern == kMemPatternWalk) {
    const uint32_t g_lo = c_lo * 4u + s_lo;  // lo32(4c) + lo32(seed)
    for (int k = 0; k < 4; ++k) out.d[k] = 1u << ((g_lo + (uint32_t)k) & 31u);
  } else {  // kMemPatternChecker: only the low bit of c + k + seed matters
    const uint32_t par = (c_lo + s_lo) & 1u;
    const uint32_t even = par ? 0x55555555u : 0xAAAAAAAAu;  // k = 0, 2
    out.d[0] = even;
    out.d[1] = ~even;
    out.d[2] = even;
    out.d[3] = ~even;
  }
  if (invert) {
    for (int k = 0; k < 4; ++k) out.d[k] = ~out.d[k];
  }
  return out;
}

K3_MEMTEST_HD inline MemCell memtest_cell(const MemSpec& spec, uint64_t c) {
  return memtest_cell(spec.pattern, spec.seed, spec.invert != 0, c);
}

}  // namespace k3samd_kern
