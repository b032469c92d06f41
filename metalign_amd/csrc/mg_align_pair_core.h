// mg_align_pair_core.h — the rules of the aligner's paired-end mode (--align_pairs interleaved; metalign_amd/align.py: place_of,
// concordant, rescue_window, select_pair and pair_flag are the definition): what the kernels of mg_align.hip decide per alignment,
// per anchor and per pair.
//
//   PairAln              what the rules read of an alignment: its accession row, strand, score and the place [u, v) of its whole
//                        oriented read on the reference, clips included: u = pos0 - b, v = pos0 + span + (L - e)
//   pair_aln()           that, from an alignment's fields and its read's length
//   concordant()         one accession, different strands, and with f the strand-0 and r the strand-1 alignment:
//                        u(f) <= u(r), v(f) <= v(r), v(r) - u(f) <= I
//   rescue_window()      the diagonals [lo, hi] of strand 1 - s on which an anchor (s, d) of a mate of L bases seeks its partner of
//                        L' bases, clipped to [1 - L', n - 1]; false for an empty range
//   pair_best()          the best concordant pair of two lists: the highest sum of scores, then the smallest place in the first
//                        list, then in the second
//   pair_partner()       the best score among the entries of the other list that are concordant with one alignment
//   pair_secondary_ok()  100 (x.score + partner) >= sec_pct * best
//   pair_flag()          a record's FLAG bits
//
// Written so that the SAME code compiles for the host (tests/host_align_pair_check.cpp) and for gfx950.  A list is reached through
// an accessor (`list(i)` = entry i as a PairAln).
#pragma once
#include <stdint.h>

#include "mg_align_core.h"

namespace mga {

constexpr uint32_t kMaxInsert = 8192, kMaxRescue = 8, kPairList = 16;

struct PairAln {
  uint32_t a, strand, score;
  int64_t u, v;
};

MGA_HD PairAln pair_aln(uint32_t a, uint32_t strand, uint32_t score, uint32_t pos0, uint32_t span, uint32_t b, uint32_t e, uint32_t L) {
  PairAln x;
  x.a = a;
  x.strand = strand;
  x.score = score;
  x.u = (int64_t)pos0 - (int64_t)b;
  x.v = (int64_t)pos0 + (int64_t)span + ((int64_t)L - (int64_t)e);
  return x;
}

MGA_HD bool concordant(const PairAln& x, const PairAln& y, int64_t I) {
  if (x.a != y.a || x.strand == y.strand) return false;
  const PairAln& f = x.strand == 0 ? x : y;
  const PairAln& r = x.strand == 0 ? y : x;
  return f.u <= r.u && f.v <= r.v && r.v - f.u <= I;
}

MGA_HD bool rescue_window(uint32_t strand, int64_t d, int64_t L, int64_t Lp, int64_t n, int64_t I, int64_t* lo, int64_t* hi) {
  int64_t l, h;
  if (strand == 0) {
    l = d + (L > Lp ? L - Lp : 0);
    h = d + I - Lp;
  } else {
    l = d + L - I;
    h = d + (L < Lp ? L - Lp : 0);
  }
  if (l < 1 - Lp) l = 1 - Lp;
  if (h > n - 1) h = n - 1;
  *lo = l;
  *hi = h;
  return l <= h;
}

template <class A, class B>
MGA_HD bool pair_best(const A& first, uint32_t n1, const B& second, uint32_t n2, int64_t I, uint32_t* bi, uint32_t* bj, uint32_t* best) {
  bool any = false;
  uint32_t top = 0;
  for (uint32_t i = 0; i < n1; ++i) {
    const PairAln x = first(i);
    for (uint32_t j = 0; j < n2; ++j) {
      const PairAln y = second(j);
      if (!concordant(x, y, I)) continue;
      if (!any || x.score + y.score > top) {
        any = true;
        top = x.score + y.score;
        *bi = i;
        *bj = j;
      }
    }
  }
  *best = top;
  return any;
}

// the best score among the other list's entries concordant with x; false: none is
template <class B> MGA_HD bool pair_partner(const PairAln& x, const B& other, uint32_t n, int64_t I, uint32_t* score) {
  bool any = false;
  uint32_t top = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const PairAln y = other(j);
    if (!concordant(x, y, I)) continue;
    if (!any || y.score > top) top = y.score;
    any = true;
  }
  *score = top;
  return any;
}

MGA_HD bool pair_secondary_ok(uint32_t score, uint32_t partner, uint32_t best, uint32_t sec_pct) {
  return 100u * (score + partner) >= sec_pct * best;
}

// mate 0 / 1; t: 0 the primary; partner_has: the other mate has a record, partner_strand: its primary's strand
MGA_HD uint32_t pair_flag(uint32_t mate, uint32_t t, uint32_t strand, bool partner_has, uint32_t partner_strand, bool proper) {
  return 1u + (proper ? 2u : 0u) + (partner_has ? 0u : 8u) + 16u * strand + (partner_has && partner_strand ? 32u : 0u) +
         (mate ? 128u : 64u) + (t ? 256u : 0u);
}

}  // namespace mga
