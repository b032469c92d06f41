// mg_coverage_core.h — the arithmetic of placing an alignment on its reference (--coverage; metalign_amd/coverage.py is the
// definition): what the tokenisers' place kernels (mg_ingest.hip, mg_bam.hip) and the coverage kernels (mg_coverage.hip) decide
// per record.
//
//   field()        field k of line.strip().split(): the k-th maximal run of non-white-space bytes of [beg, end)
//   pos_of()       POS: 1 to 10 ASCII digits with 1 <= POS <= 2^31 - 1 -> pos0 = POS - 1; anything else is no error, the record
//                  is just not placed
//   cigar_span()   the reference bases a CIGAR string consumes: the lengths of its M, D, N and X ops (the tokeniser has already
//                  refused every byte that is neither a digit nor a letter); at most 2^32 - 1, a larger sum stays there
//   bam_span()     the same over a BAM record's packed ops: codes 0 (M), 2 (D), 3 (N), 8 (X)
//   counts()       clean_read_hits keeps the record (scripts/map_and_profile.py:130-147), by the very expression of stage C's
//                  make_desc (mg_profile.hip)
//   clipped()      the length of [pos0, min(pos0 + span, L)); 0: not placed (span 0, or pos0 >= L)
//   interval()     bits [b, e) of an accession's bitmap, e > b, in 32-bit words: first word, its mask, last word, its mask
//   word_mask()    the mask of word w of that interval
//   owner_of()     the accession that owns an offset, by binary search in the accessions' ascending offsets (the coverage, depth and
//                  variants kernels); owner_from(): the same by walking on from an accession before it
//
// Written so that the SAME code compiles for the host (tests/host_coverage_check.cpp) and for gfx950.  Memory is reached through
// an accessor (`m[i]` = byte i).
#pragma once
#include <stdint.h>

#include "../../include/metalign_hip.h"

#if defined(__HIPCC__)
#define MGV_HD __host__ __device__ inline
#else
#define MGV_HD inline
#endif

namespace mgv {

constexpr uint64_t kMaxPos = 0x7fffffffull, kMaxSpan = 0xffffffffull;

MGV_HD bool is_ws(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }  // str.split()'s, as the parser's
MGV_HD bool is_alpha(uint32_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

// Field k (0-based) of the line [beg, end) -> [*fb, *fe); false when the line has fewer fields.
template <class M> MGV_HD bool field(const M& m, uint64_t beg, uint64_t end, int k, uint64_t* fb, uint64_t* fe) {
  uint64_t p = beg;
  for (int f = 0;; ++f) {
    while (p < end && is_ws(m[p])) ++p;
    if (p >= end) return false;
    const uint64_t b = p;
    while (p < end && !is_ws(m[p])) ++p;
    if (f == k) { *fb = b; *fe = p; return true; }
  }
}

template <class M> MGV_HD bool pos_of(const M& m, uint64_t b, uint64_t e, uint32_t* pos0) {
  if (e <= b || e - b > 10) return false;
  uint64_t v = 0;
  for (uint64_t p = b; p < e; ++p) {
    const uint32_t c = m[p];
    if (c < '0' || c > '9') return false;
    v = v * 10 + (c - '0');
  }
  if (v < 1 || v > kMaxPos) return false;
  *pos0 = (uint32_t)(v - 1);
  return true;
}

template <class M> MGV_HD uint32_t cigar_span(const M& m, uint64_t b, uint64_t e) {
  uint64_t span = 0, cur = 0;
  for (uint64_t p = b; p < e; ++p) {
    const uint32_t c = m[p];
    if (is_alpha(c)) {
      if (c == 'M' || c == 'D' || c == 'N' || c == 'X') span += cur;
      if (span > kMaxSpan) span = kMaxSpan;
      cur = 0;
    } else if (c >= '0' && c <= '9') {
      cur = cur * 10 + (c - '0');
      if (cur > kMaxSpan) cur = kMaxSpan;
    }
  }
  return (uint32_t)span;
}

// ops: ncig little-endian u32 at m[cig ..], len << 4 | code
template <class M> MGV_HD uint32_t bam_span(const M& m, uint64_t cig, uint32_t ncig) {
  uint64_t span = 0;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint64_t o = cig + 4ull * i;
    const uint32_t v = (uint32_t)m[o] | ((uint32_t)m[o + 1] << 8) | ((uint32_t)m[o + 2] << 16) | ((uint32_t)m[o + 3] << 24);
    const uint32_t op = v & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 8) span += v >> 4;
  }
  return (uint32_t)(span > kMaxSpan ? kMaxSpan : span);
}

// The place of a SAM line [beg, end) the tokeniser retained (it has 6 fields or more): POS is field 3, the CIGAR field 5.
template <class M> MGV_HD mg_aln_place place_of_line(const M& m, uint64_t beg, uint64_t end) {
  mg_aln_place pl;
  pl.pos0 = 0;
  pl.span = 0;
  uint64_t pb, pe, cb, ce;
  uint32_t pos0 = 0;
  if (!field(m, beg, end, 3, &pb, &pe) || !pos_of(m, pb, pe, &pos0)) return pl;
  if (!field(m, pe, end, 1, &cb, &ce)) return pl;  // (field 5: the second one behind POS)
  const uint32_t span = cigar_span(m, cb, ce);
  if (span) { pl.pos0 = pos0; pl.span = span; }
  return pl;
}

// The place of the BAM record whose QNAME starts at qn (the record at qn - 36: block_size and the 32 fixed bytes in front of it).
template <class M> MGV_HD mg_aln_place place_of_bam(const M& m, uint64_t qn) {
  mg_aln_place pl;
  pl.pos0 = 0;
  pl.span = 0;
  const uint64_t p = qn - 36;
  const int32_t pos = (int32_t)((uint32_t)m[p + 8] | ((uint32_t)m[p + 9] << 8) | ((uint32_t)m[p + 10] << 16) | ((uint32_t)m[p + 11] << 24));
  const uint32_t lrn = m[p + 12], ncig = (uint32_t)m[p + 16] | ((uint32_t)m[p + 17] << 8);
  if (pos < 0 || pos > (int32_t)(kMaxPos - 1)) return pl;  // (POS = pos + 1 <= 2^31 - 1, as for the text)
  const uint32_t span = bam_span(m, qn + lrn, ncig);
  if (span) { pl.pos0 = (uint32_t)pos; pl.span = span; }
  return pl;
}

MGV_HD bool counts(const mg_aln_rec& r, double pct_id) {
  const uint32_t fl = r.flag_len & MG_REC_FLAG_MASK;
  const bool rej = ((double)r.matched / (double)r.total < pct_id) || (fl & 2048u);
  return !rej;
}

MGV_HD uint64_t clipped(uint32_t pos0, uint32_t span, uint64_t L) {
  if (span == 0 || (uint64_t)pos0 >= L) return 0;
  const uint64_t e = (uint64_t)pos0 + span;
  return (e < L ? e : L) - pos0;
}

// The accession of offset t (a bitmap word, a depth slot or window, a site): the last a with off[a] <= t < off[a + 1]; off has
// n + 1 ascending entries, off[n] > t.
template <class O> MGV_HD uint32_t owner_of(const O& off, uint32_t n, uint64_t t) {
  uint32_t lo = 0, hi = n;  // the first index in [0, n] whose offset is above t
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}
// The same for a walk: a owned an offset at or below t; steps over the accessions that own nothing.  n when t = off[n].
template <class O> MGV_HD uint32_t owner_from(const O& off, uint32_t n, uint32_t a, uint64_t t) {
  while (a < n && off[a + 1] <= t) ++a;
  return a;
}

MGV_HD void interval(uint64_t b, uint64_t e, uint64_t* w0, uint32_t* m0, uint64_t* w1, uint32_t* m1) {
  *w0 = b >> 5;
  *w1 = (e - 1) >> 5;
  *m0 = 0xffffffffu << (uint32_t)(b & 31);
  *m1 = 0xffffffffu >> (31u - (uint32_t)((e - 1) & 31));
}

MGV_HD uint32_t word_mask(uint64_t w, uint64_t w0, uint32_t m0, uint64_t w1, uint32_t m1) {
  uint32_t m = 0xffffffffu;
  if (w == w0) m &= m0;
  if (w == w1) m &= m1;
  return m;
}

}  // namespace mgv
