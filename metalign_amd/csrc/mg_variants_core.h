// mg_variants_core.h — the arithmetic of piling an alignment's bases on its reference and of judging a site (--variants,
// --variant_sites; metalign_amd/variants.py is the definition): what the variants kernels (mg_variants.hip) decide per record and
// per site, and the scalar walks that turn a SAM line or a BAM record into the 4-bit codes of a batch's pool.
//
//   code_of()        a SEQ byte: A a 0, C c 1, G g 2, T t 3, every other byte kOther = 4
//   bam_code_of()    a BAM SEQ nibble: 1, 2, 4, 8 are A, C, G, T, every other value kOther
//   sam_pile_span()  a retained SAM line's CIGAR [cb, ce) and SEQ [sb, se): the number of codes it piles — its span (the lengths of
//                    M, D, N and X) — or 0 when it cannot be piled: span 0 or above kMaxPileSpan, SEQ `*`, or the query bases its
//                    M, X, I and S ops consume are not len(SEQ)
//   sam_pile_walk()  the codes themselves, in reference order, to a sink: M and X give the next query bases' codes, I and S step
//                    over query bases, D and N give kGap, every other letter (H, P, a lower-case one) gives nothing.  Only for a
//                    line sam_pile_span() accepted: then every SEQ byte it reads lies in [sb, se).
//   bam_pile_span()  the same for the BAM record whose QNAME starts at qn (decode() has judged it complete and retained it): packed
//   bam_pile_walk()  ops (codes 0 M, 1 I, 2 D, 3 N, 4 S, 8 X; 5 H, 6 P and 7 = give nothing), 4-bit SEQ with the high nibble
//                    first, l_seq == 0 is `*`.  A record whose ops or SEQ would reach its end is not piled.
//   NibblePacker     a sink that packs codes two per byte, the low nibble first; flush() writes a last odd code with a 0 above it
//   site_of()        one site's four counts against (D, C, F): its depth, whether it is callable, its major allele (ties to the
//                    lowest code), the mask of its variant alleles, d (d - 1) and d (d - 1) - sum n_i (n_i - 1)
//   diff_of()        one site's four counts against its reference code (--ani, --vcf; metalign_amd/refdiff.py), over site_of()
//   consensus_char() one site's character in the consensus sequence (--consensus; metalign_amd/consensus.py), over site_of()
//   text_bytes()     the bytes of a sequence as text of lines of `width` bases; text_at(): the inverse layout map, which byte of the
//                    text is a newline and which site every other byte shows; 64-bit throughout
//
// Written so that the SAME code compiles for the host (tests/host_variants_check.cpp) and for gfx950.  Memory is reached through an
// accessor (`m[i]` = byte i).  No byte at or behind the end of a line or record is read.
#pragma once
#include <stdint.h>

#include "../../include/metalign_hip.h"
#include "mg_bam_core.h"
#include "mg_coverage_core.h"

namespace mgvar {

constexpr uint32_t kOther = 4, kGap = 5;
constexpr uint32_t kMaxPileSpan = MG_MAX_PILE_SPAN;

MGV_HD uint32_t code_of(uint32_t c) {
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return kOther;
  }
}

MGV_HD uint32_t bam_code_of(uint32_t nib) { return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : kOther; }

// the sum of the lengths of a CIGAR string's query-consuming ops (M, X, I, S); saturates at 2^32 - 1
template <class M> MGV_HD uint32_t cigar_query(const M& m, uint64_t b, uint64_t e) {
  uint64_t q = 0, cur = 0;
  for (uint64_t p = b; p < e; ++p) {
    const uint32_t c = m[p];
    if (mgv::is_alpha(c)) {
      if (c == 'M' || c == 'X' || c == 'I' || c == 'S') q += cur;
      if (q > mgv::kMaxSpan) q = mgv::kMaxSpan;
      cur = 0;
    } else if (c >= '0' && c <= '9') {
      cur = cur * 10 + (c - '0');
      if (cur > mgv::kMaxSpan) cur = mgv::kMaxSpan;
    }
  }
  return (uint32_t)q;
}

template <class M> MGV_HD uint32_t sam_pile_span(const M& m, uint64_t cb, uint64_t ce, uint64_t sb, uint64_t se) {
  const uint32_t span = mgv::cigar_span(m, cb, ce);
  if (span == 0 || span > kMaxPileSpan) return 0;
  if (se <= sb || (se - sb == 1 && m[sb] == '*')) return 0;
  if ((uint64_t)cigar_query(m, cb, ce) != se - sb) return 0;
  return span;
}

template <class M, class Sink> MGV_HD void sam_pile_walk(const M& m, uint64_t cb, uint64_t ce, uint64_t sb, Sink& sink) {
  uint64_t cur = 0, q = sb;
  for (uint64_t p = cb; p < ce; ++p) {
    const uint32_t c = m[p];
    if (mgv::is_alpha(c)) {
      if (c == 'M' || c == 'X') {
        for (uint64_t i = 0; i < cur; ++i) sink.put(code_of(m[q + i]));
        q += cur;
      } else if (c == 'I' || c == 'S') {
        q += cur;
      } else if (c == 'D' || c == 'N') {
        for (uint64_t i = 0; i < cur; ++i) sink.put(kGap);
      }
      cur = 0;
    } else if (c >= '0' && c <= '9') {
      cur = cur * 10 + (c - '0');  // (at most kMaxPileSpan or len(SEQ) where it is used: sam_pile_span() has seen the sums)
      if (cur > mgv::kMaxSpan) cur = mgv::kMaxSpan;
    }
  }
}

// Where the ops and the SEQ of the BAM record at qn - 36 lie; false when they would reach behind its end.
template <class M> MGV_HD bool bam_parts(const M& m, uint64_t qn, uint64_t* cig, uint32_t* ncig, uint64_t* seq, uint32_t* lseq) {
  const uint64_t p = qn - 36;
  const uint64_t end = p + 4 + (uint64_t)mgb::ld32(m, p);
  *cig = qn + m[p + 12];
  *ncig = mgb::ld16(m, p + 16);
  *lseq = mgb::ld32(m, p + 20);
  *seq = *cig + 4ull * *ncig;
  return *seq + ((uint64_t)*lseq + 1) / 2 <= end;
}

template <class M> MGV_HD uint32_t bam_pile_span(const M& m, uint64_t qn) {
  uint64_t cig, seq;
  uint32_t ncig, lseq;
  if (!bam_parts(m, qn, &cig, &ncig, &seq, &lseq) || lseq == 0) return 0;
  const uint32_t span = mgv::bam_span(m, cig, ncig);
  if (span == 0 || span > kMaxPileSpan) return 0;
  uint64_t q = 0;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = mgb::ld32(m, cig + 4ull * i), op = v & 15u;
    if (op == 0 || op == 1 || op == 4 || op == 8) q += v >> 4;
  }
  return q == lseq ? span : 0;
}

template <class M, class Sink> MGV_HD void bam_pile_walk(const M& m, uint64_t qn, Sink& sink) {
  uint64_t cig, seq;
  uint32_t ncig, lseq;
  (void)bam_parts(m, qn, &cig, &ncig, &seq, &lseq);
  uint64_t q = 0;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = mgb::ld32(m, cig + 4ull * i), op = v & 15u, len = v >> 4;
    if (op == 0 || op == 8) {
      for (uint64_t j = q; j < q + len; ++j) sink.put(bam_code_of((m[seq + (j >> 1)] >> ((j & 1) ? 0 : 4)) & 15u));
      q += len;
    } else if (op == 1 || op == 4) {
      q += len;
    } else if (op == 2 || op == 3) {
      for (uint32_t j = 0; j < len; ++j) sink.put(kGap);
    }
  }
}

// out[at + j / 2] takes code j: `Out` is anything with `out[i] = byte`.
template <class Out> struct NibblePacker {
  Out out;
  uint64_t at;
  uint32_t n = 0, low = 0;
  MGV_HD NibblePacker(Out o, uint64_t a) : out(o), at(a) {}
  MGV_HD void put(uint32_t code) {
    if (n & 1u) out[at + (n >> 1)] = (uint8_t)(low | (code << 4));
    else low = code;
    ++n;
  }
  MGV_HD void flush() {
    if (n & 1u) out[at + (n >> 1)] = (uint8_t)low;
  }
};

// code j of the entry whose codes start at pool[off]
template <class M> MGV_HD uint32_t code_at(const M& pool, uint64_t off, uint64_t j) {
  return ((uint32_t)pool[off + (j >> 1)] >> (4u * (uint32_t)(j & 1))) & 15u;
}

struct Site {
  uint64_t d, pairs, discordant;  // pairs and discordant: of a callable site, 0 otherwise
  uint32_t major, variants;       // variants: bit a set for a variant allele a
  bool callable_, polymorphic;
};

MGV_HD Site site_of(const uint32_t n[4], uint32_t min_depth, uint32_t min_count, uint32_t permille) {
  Site s;
  s.d = (uint64_t)n[0] + n[1] + n[2] + n[3];
  s.pairs = s.discordant = 0;
  s.major = s.variants = 0;
  s.callable_ = s.d >= min_depth;
  s.polymorphic = false;
  if (!s.callable_) return s;
  for (uint32_t a = 1; a < 4; ++a)
    if (n[a] > n[s.major]) s.major = a;
  uint64_t same = 0;
  for (uint32_t a = 0; a < 4; ++a) {
    same += (uint64_t)n[a] * (n[a] ? n[a] - 1ull : 0ull);
    if (a != s.major && n[a] >= min_count && 1000ull * n[a] >= (uint64_t)permille * s.d) s.variants |= 1u << a;
  }
  s.pairs = s.d * (s.d - 1);
  s.discordant = s.pairs - same;
  s.polymorphic = s.variants != 0;
  return s;
}

// One site against its reference code r (--ani, --vcf; metalign_amd/refdiff.py is the definition), over site_of(): compared — the
// site is callable and r < 4; ref_other — callable and r is kOther; con_sub — compared and the major allele is not r; pop_sub —
// compared and r is neither the major nor a variant allele; emitted — compared and some present allele is not r.
struct Diff {
  bool compared, ref_other, con_sub, pop_sub, emitted;
};

MGV_HD Diff diff_of(const uint32_t n[4], uint32_t r, uint32_t min_depth, uint32_t min_count, uint32_t permille) {
  const Site s = site_of(n, min_depth, min_count, permille);
  Diff d{false, false, false, false, false};
  if (!s.callable_) return d;
  if (r >= kOther) {
    d.ref_other = true;
    return d;
  }
  const uint32_t present = (1u << s.major) | s.variants;
  d.compared = true;
  d.con_sub = s.major != r;
  d.pop_sub = ((present >> r) & 1u) == 0;
  d.emitted = (present & ~(1u << r)) != 0;
  return d;
}

// ---- the consensus text (--consensus; metalign_amd/consensus.py is the definition) --------------------------------------------

constexpr uint64_t pack8(const char* s) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return v;
}

// "-ACMGRSVTWYHKDBN"[mask], bits A = 1, C = 2, G = 4, T = 8 (two 64-bit constants: no table in memory)
MGV_HD uint8_t iupac_of(uint32_t mask) {
  constexpr uint64_t lo = pack8("-ACMGRSV"), hi = pack8("TWYHKDBN");
  return (uint8_t)(((mask & 8u) ? hi : lo) >> (8u * (mask & 7u)));
}

// One site's character: N below min_depth; else the major allele's letter, or (iupac) the code of the major and the variant alleles.
MGV_HD uint8_t consensus_char(const uint32_t n[4], uint32_t min_depth, uint32_t min_count, uint32_t permille, bool iupac) {
  const Site s = site_of(n, min_depth, min_count, permille);
  if (!s.callable_) return 'N';
  return iupac_of((1u << s.major) | (iupac ? s.variants : 0u));
}

// The bytes of a sequence of L bases as text: a newline behind every `width` bases and behind the last one (width >= 1).
MGV_HD uint64_t text_bytes(uint64_t L, uint32_t width) { return L + (L + width - 1) / width; }

struct TextAt {
  bool newline;
  uint64_t site;  // (of a byte that is no newline)
};
// Byte i of a text of lines of `width` bases: the newline that closes a full line, or the site it shows.  (A 32-bit division
// where i allows it: the 64-bit one is a long loop on the device.)
MGV_HD TextAt text_at(uint64_t i, uint32_t width) {
  const uint64_t w1 = (uint64_t)width + 1;
  uint64_t line, col;
  if ((i >> 32) == 0) {
    line = (uint32_t)i / (uint32_t)w1;
    col = (uint32_t)i % (uint32_t)w1;
  } else {
    line = i / w1;
    col = i % w1;
  }
  return TextAt{col == width, line * width + col};
}
// ... of the text of a sequence of L bases, i < text_bytes(L, width): the newline behind a short last line stands where site L
// would.  The inverse of the layout: site s is byte s + s / width.
MGV_HD TextAt text_at(uint64_t i, uint32_t width, uint64_t L) {
  TextAt t = text_at(i, width);
  t.newline = t.newline || t.site >= L;
  return t;
}

}  // namespace mgvar
