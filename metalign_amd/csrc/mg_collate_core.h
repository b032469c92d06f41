// mg_collate_core.h — what collating alignment records by read (mg_collate.hip) decides per record: the 128-bit key of a QNAME
// and the class of a record inside its read.
//
// Stage C closes a read when the QNAME changes (scripts/map_and_profile.py:220), so a coordinate-sorted file has to be regrouped
// first.  The definition is metalign_amd/collate.py (collated_lines); on the device names are compared through
//
//   qname_key()   both halves of MurmurHash3_x64_128 (the function mg_kmer.h specialises on k, here for any length) over the QNAME
//                 bytes with the fixed seed kSeed: lo = h1, hi = h2.  Two names are the same read exactly when BOTH halves agree;
//                 two DIFFERENT names that agree in all 128 bits would be merged (below n^2 / 2^129 for n names: DESIGN.md §4).
//   rec_class()   mate2 << 1 | notprimary of a FLAG: mate 2 = paired (1) and last (128) and not first (64) — the reference's
//                 `pair2 and not pair1`, its intersect_read_hits slices [:pair1maps] so read-1 lines come first; not primary =
//                 secondary (0x100) or supplementary (0x800).
//
// Written so that the SAME code compiles for the host (tests/host_collate_check.cpp) and for gfx950.  Bytes are read one at a
// time: a QNAME starts at any address.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MGC_HD __host__ __device__ inline
#else
#define MGC_HD inline
#endif

namespace mgc {

constexpr uint32_t kSeed = 0x6d67636fu;  // "mgco"; MurmurHash3 seeds are 32 bits wide
constexpr uint64_t kC1 = 0x87c37b91114253d5ULL, kC2 = 0x4cf5ad432745937fULL;

MGC_HD uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

MGC_HD uint64_t fmix(uint64_t v) {
  v ^= v >> 33;
  v *= 0xff51afd7ed558ccdULL;
  v ^= v >> 33;
  v *= 0xc4ceb9fe1a85ec53ULL;
  v ^= v >> 33;
  return v;
}

// bytes [o, o + len) of m, len <= 8, little-endian
template <class M> MGC_HD uint64_t ld_le(const M& m, uint64_t o, uint32_t len) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < len; ++i) v |= (uint64_t)(uint8_t)m[o + i] << (8 * i);
  return v;
}

// m[o .. o + n): the name.  M is anything with operator[] (a pointer; the host test's checked array).
template <class M> MGC_HD void qname_key(const M& m, uint64_t o, uint32_t n, uint64_t* lo, uint64_t* hi) {
  uint64_t h1 = kSeed, h2 = kSeed;
  const uint32_t full = n & ~15u;
  for (uint32_t b = 0; b < full; b += 16) {
    uint64_t k1 = ld_le(m, o + b, 8), k2 = ld_le(m, o + b + 8, 8);
    k1 *= kC1; k1 = rotl(k1, 31); k1 *= kC2; h1 ^= k1;
    h1 = rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= kC2; k2 = rotl(k2, 33); k2 *= kC1; h2 ^= k2;
    h2 = rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
  }
  const uint32_t tail = n - full;
  if (tail > 8) {
    uint64_t k2 = ld_le(m, o + full + 8, tail - 8);
    k2 *= kC2; k2 = rotl(k2, 33); k2 *= kC1; h2 ^= k2;
  }
  if (tail > 0) {
    uint64_t k1 = ld_le(m, o + full, tail > 8 ? 8 : tail);
    k1 *= kC1; k1 = rotl(k1, 31); k1 *= kC2; h1 ^= k1;
  }
  h1 ^= n; h2 ^= n;
  h1 += h2; h2 += h1;
  h1 = fmix(h1); h2 = fmix(h2);
  h1 += h2; h2 += h1;
  *lo = h1;
  *hi = h2;
}

MGC_HD uint32_t rec_class(uint32_t flag) {
  const uint32_t mate2 = ((flag & 1u) && (flag & 128u) && !(flag & 64u)) ? 1u : 0u;
  const uint32_t notprimary = (flag & 0x900u) ? 1u : 0u;
  return mate2 << 1 | notprimary;
}

// The key the second sort orders by: the read's group (the file index of its first retained line), then the class.
MGC_HD uint64_t final_key(uint64_t gid, uint32_t flag) { return gid << 2 | rec_class(flag); }

}  // namespace mgc
