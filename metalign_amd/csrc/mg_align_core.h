// mg_align_core.h — the per-position rules of the seed-and-extend aligner (--aligner device; metalign_amd/align.py is the
// definition): what the kernels of mg_align.hip decide per base, per k-mer position, per column and per alignment.
//
//   code_of() / comp()   a base's code (A a 0, C c 1, G g 2, T t 3, every other byte 4) and a code's complement
//   fmix64()             the key of a canonical k-mer value
//   Roll / push() / key_of()   the forward and reverse-complement values of the last k bases, one base at a time; the key and the
//                        strand bit of the k-mer that ends at the last base pushed
//   minimizer_at()       whether k-mer position p of a sequence is a minimizer: the position some window [s, min(s + w, m)) chooses
//                        (smallest key, the leftmost among equals)
//   Scan / step()        the extension's scan, one column at a time: the first segment to reach the highest score wins
//   nm_of()              the columns of a segment that did not add 1, from its span and score
//   overlaps() / secondary_ok()   the selection's two rules
//
// Written so that the SAME code compiles for the host (tests/host_align_check.cpp) and for gfx950.  A sequence is reached through
// an accessor (`code(i)` = the code of base i).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MGA_HD __host__ __device__ inline
#else
#define MGA_HD inline
#endif

namespace mga {

constexpr uint32_t kOther = 4;
constexpr uint32_t kMaxRead = 1024;  // a longer read has no candidates
constexpr uint32_t kMinK = 11, kMaxK = 31, kMaxW = 32, kMaxSecondary = 15;

MGA_HD uint32_t code_of(uint32_t c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return kOther;
  }
}

MGA_HD uint32_t comp(uint32_t c) { return c < 4 ? 3u - c : kOther; }

MGA_HD uint64_t fmix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

struct Roll {
  uint64_t f = 0, r = 0;
  uint32_t valid = 0;  // the bases since the last code 4, at most k
};

MGA_HD void push(Roll& s, uint32_t code, uint32_t k) {
  if (code < 4) {
    s.f = ((s.f << 2) | code) & ((1ull << (2 * k)) - 1);
    s.r = (s.r >> 2) | ((uint64_t)(3u - code) << (2 * (k - 1)));
    if (s.valid < k) ++s.valid;
  } else {
    s.f = s.r = 0;
    s.valid = 0;
  }
}

struct Key {
  uint64_t key;
  uint32_t strand;
  bool ok;  // false: the k-mer holds a code 4 (or fewer than k bases were pushed)
};

MGA_HD Key key_of(const Roll& s, uint32_t k) {
  Key o;
  o.ok = s.valid >= k;
  o.strand = s.f < s.r ? 0u : 1u;
  o.key = fmix64(s.f < s.r ? s.f : s.r);
  return o;
}

// Position p < m = n - k + 1 of a sequence of n >= k bases.  L = the positions directly left of p (within w - 1) whose key is
// above p's or that have none, R = those directly right of it whose key is not below: the window [s, e) chooses p iff
// p - s <= L and e - 1 - p <= R, and the smallest s the left side allows is the one the right side likes best.
template <class C> MGA_HD bool minimizer_at(const C& code, uint64_t n, uint64_t p, uint32_t k, uint32_t w, Key* out) {
  const uint64_t m = n - k + 1;
  Roll s;
  for (uint64_t i = p; i < p + k; ++i) push(s, code(i), k);
  const Key kp = key_of(s, k);
  *out = kp;
  if (!kp.ok) return false;
  const uint64_t lo = p >= w - 1 ? p - (w - 1) : 0;
  const uint64_t hi = p + w - 1 < m ? p + w - 1 : m - 1;
  uint64_t L = p - lo, R = hi - p;
  Roll t;
  for (uint64_t i = lo; i < hi + k; ++i) {
    push(t, code(i), k);
    if (i < lo + k - 1) continue;
    const uint64_t q = i - (k - 1);
    if (q == p) continue;
    const Key kq = key_of(t, k);
    if (!kq.ok) continue;
    if (q < p) {
      if (kq.key <= kp.key) L = p - 1 - q;
    } else if (kq.key < kp.key) {
      R = q - p - 1;
      break;
    }
  }
  const uint64_t s_hi = m > w ? (p < m - w ? p : m - w) : 0;
  const uint64_t s0 = p - L > lo ? p - L : lo;
  if (s0 > s_hi) return false;
  const uint64_t e = s0 + w < m ? s0 + w : m;
  return e - 1 - p <= R;
}

struct Scan {
  int32_t cur = 0, start = 0, best = 0, b = 0, e = 0;
};

// column j: outside the accession, or inside and adding 1 (match) or subtracting P
MGA_HD void step(Scan& s, int32_t j, bool inside, bool match, int32_t P) {
  if (!inside) {
    s.cur = 0;
    s.start = j + 1;
    return;
  }
  s.cur += match ? 1 : -P;
  if (s.cur <= 0) {
    s.cur = 0;
    s.start = j + 1;
  } else if (s.cur > s.best) {
    s.best = s.cur;
    s.b = s.start;
    s.e = j + 1;
  }
}

// score = matches - P (span - matches): the columns that did not add 1
MGA_HD uint32_t nm_of(uint32_t span, uint32_t score, uint32_t P) { return (span - score) / (P + 1u); }

MGA_HD bool overlaps(uint32_t a0, uint32_t s0, uint32_t pos0, uint32_t end0, uint32_t a1, uint32_t s1, uint32_t pos1, uint32_t end1) {
  return a0 == a1 && s0 == s1 && pos0 < end1 && pos1 < end0;
}

MGA_HD bool secondary_ok(uint32_t score, uint32_t best, uint32_t sec_pct) { return score * 100u >= best * sec_pct; }

}  // namespace mga
