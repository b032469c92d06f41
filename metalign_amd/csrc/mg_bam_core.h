// mg_bam_core.h — BAM alignment records (SAM specification §4.2) as the device finds and decodes them (mg_bam.hip).
//
// The reference reads SAM text only (scripts/map_and_profile.py:201-217), so a BAM record is defined THROUGH its SAM rendering:
// it must give the record (or the exception) that the line `samtools view` prints for it gives through the SAM tokeniser.  This
// header holds the per-record logic, written so that the SAME code compiles for the host (tests/host_bam_check.cpp runs it
// against a Python rendering where there is no GPU) and for gfx950:
//
//   check()   is the record at p a plausible one?  block_size covers the fixed part, QNAME, CIGAR, SEQ and QUAL; refID and
//             next_refID in [-1, n_ref); QNAME NUL-terminated; the record inside [0, n).  Every load is bounds-checked against
//             n BEFORE it is made: a corrupt block_size never reads outside the range.
//   walk()    the block_size chain from an entry over the records that START before a stop offset (one chunk of a piece).
//   decode()  one record -> mg_aln_rec (without the new-read bit), its QNAME span, retained or not, or an error kind.
//
// A BAM READS file (stages A / B) is defined through `samtools fastq` with its default filter (-F 0x900):
//   seq_kept()   a record is a read unless it is secondary (0x100) or supplementary (0x800);
//   kept_len()   its length: l_seq (0 for SEQ '*'), 0 for a record that is not kept;
//   seq_base()   base j of the read, in the read's own orientation: the 4-bit code through "=ACMGRSVTWYHKDBN", a record with 0x10
//                set read backwards through the complement of each code (the code's four bits reversed: A<->T, C<->G, M<->K,
//                R<->Y, V<->B, H<->D; S, W, N and '=' stay).
//
// Memory is reached through an accessor (`m[i]` = byte i of the range), so that the host test can run the same code on a
// plain array.
#pragma once
#include <stdint.h>

#include "../../include/metalign_hip.h"

#if defined(__HIPCC__)
#define MGB_HD __host__ __device__ inline
#else
#define MGB_HD inline
#endif

namespace mgb {

// Error kinds: 1..5 are the SAM tokeniser's (include/metalign_hip.h), 6 and 7 are BAM's own.
enum Kind : uint32_t {
  kNone = 0, kKey = 1, kIndex = 2, kValue = 3, kZeroDiv = 4, kOverflow = 5,
  kHost = 6,     // the SAM rendering of the record is not decided here (a QNAME / RNAME that is not one SAM field, a float tag, ...)
  kCorrupt = 7,  // not a BAM record, or one this package does not take (a CIGAR kept in a CG tag)
};

constexpr uint32_t kFixed = 32;                 // refID .. tlen
constexpr uint32_t kMinRecord = 4 + kFixed + 1;  // block_size + fixed part + the NUL of a QNAME

// ---- byte access, little-endian, unaligned ----
template <class M> MGB_HD uint32_t ld16(const M& m, uint64_t o) { return (uint32_t)m[o] | ((uint32_t)m[o + 1] << 8); }
template <class M> MGB_HD uint32_t ld32(const M& m, uint64_t o) {
  return (uint32_t)m[o] | ((uint32_t)m[o + 1] << 8) | ((uint32_t)m[o + 2] << 16) | ((uint32_t)m[o + 3] << 24);
}

enum Check : int { kOk = 0, kIncomplete = 1, kBad = 2 };

// The record at p of [0, n): kOk (*next = its end), kIncomplete (it runs past n — the unfinished tail of a piece, or a start that
// cannot be judged yet), kBad (not a record).  p <= n.
template <class M>
MGB_HD int check(const M& m, uint64_t n, uint64_t p, int32_t n_ref, uint64_t* next) {
  if (n - p < 4) return kIncomplete;
  const uint64_t bs = ld32(m, p);
  if (bs < kFixed + 1) return kBad;
  if (n - p < 4 + kFixed) return kIncomplete;
  const int32_t ref = (int32_t)ld32(m, p + 4), nref = (int32_t)ld32(m, p + 24);
  const uint32_t lrn = m[p + 12], ncig = ld16(m, p + 16), lseq = ld32(m, p + 20);
  if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref || lrn < 1) return kBad;
  if ((uint64_t)kFixed + lrn + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + lseq > bs) return kBad;
  if (n - p - 4 < bs) return kIncomplete;
  if (m[p + 4 + kFixed + lrn - 1] != 0) return kBad;  // (inside the record: bs covers it)
  *next = p + 4 + bs;
  return kOk;
}

// The chain from `entry`: the records that start before `stop` (their offsets - base to out[0 .. cap)) -> their number.
// *exit = the offset after the last of them (>= stop, unless the chain stopped early); *status = kOk, or what check() said at *exit.
template <class M>
MGB_HD uint32_t walk(const M& m, uint64_t n, int32_t n_ref, uint64_t entry, uint64_t stop, uint64_t base, uint32_t* out, uint32_t cap,
                     uint64_t* exit, int* status) {
  uint64_t p = entry;
  uint32_t cnt = 0;
  int st = kOk;
  while (p < stop) {
    uint64_t nx = 0;
    st = check(m, n, p, n_ref, &nx);
    if (st != kOk) break;
    if (cnt == cap) { st = kBad; break; }  // (cannot happen: a record is at least kMinRecord bytes and cap covers the chunk)
    if (out) out[cnt] = (uint32_t)(p - base);
    ++cnt;
    p = nx;
  }
  *exit = p;
  *status = st;
  return cnt;
}

// The speculative entry of a chunk: the first offset in [from, to) where check() says kOk; `to` if there is none.
template <class M>
MGB_HD uint64_t find(const M& m, uint64_t n, int32_t n_ref, uint64_t from, uint64_t to) {
  for (uint64_t q = from; q < to; ++q) {
    uint64_t nx;
    if (check(m, n, q, n_ref, &nx) == kOk) return q;
  }
  return to;
}

struct Decoded {
  mg_aln_rec rec;   // ref_new without the new-read bit
  uint64_t qbeg;    // QNAME span
  uint32_t qlen;
  uint32_t retained;
  uint32_t kind;
};

MGB_HD bool graph(uint32_t c) { return c >= 0x21 && c <= 0x7e; }          // one byte of one SAM field
MGB_HD bool split_ws(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }  // str.split()'s, as is_ws

// *t: an aux field's start -> the next one's.  false: the field runs past end, or its type is not one of SAM's.
template <class M>
MGB_HD bool aux_skip(const M& m, uint64_t end, uint64_t* t) {
  if (end - *t < 3) return false;
  const uint32_t ty = m[*t + 2];
  uint64_t v = *t + 3;
  uint64_t sz;
  switch (ty) {
    case 'A': case 'c': case 'C': sz = 1; break;
    case 's': case 'S': sz = 2; break;
    case 'i': case 'I': case 'f': sz = 4; break;
    case 'Z': case 'H': {
      while (v < end && m[v] != 0) ++v;
      if (v >= end) return false;
      *t = v + 1;
      return true;
    }
    case 'B': {
      if (end - v < 5) return false;
      const uint32_t sub = m[v];
      const uint64_t cnt = ld32(m, v + 1);
      const uint64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
      if (!es) return false;
      v += 5;
      sz = cnt * es;
      break;
    }
    default: return false;
  }
  if (end - v < sz) return false;
  *t = v + sz;
  return true;
}

// One complete record at p (a walk() found it) -> *o.  refmap[1 + refID] = the accession row of the reference's name (refmap[0]:
// of '*', refID -1); -1: no accession of that name (KeyError when a retained record uses it); -2: a name that is not one SAM field.
// The rules are those of the line the record renders as, through the SAM tokeniser (map_and_profile.py: _Tokeniser.feed):
//   QNAME '@...'               a header line: skipped;  a QNAME that is not one field (empty, a byte outside '!'..'~'): kHost
//   FLAG & 4, CIGAR '*'        skipped (n_cigar_op = 0 renders as '*')
//   retained:  RNAME row < 0 -> kKey;  an '=' op -> kValue (int('='));  no aux field -> kIndex (splits[11]);
//              int(first tag's value): c C s S i I always, A a digit, Z / H [+-]?[0-9]+ up to the first white space, B never,
//              f -> kHost (htslib's %g rendering);  total 0 -> kZeroDiv;  len(SEQ) or a sum too large -> kOverflow
// A CIGAR op above 8 and the long-read placeholder <l_seq>S<n>N with a CG tag are kCorrupt.  A field that would render with white
// space inside (RNEXT's name, a QUAL byte above '~') between RNAME and the first tag of a retained record: kHost.
template <class M>
MGB_HD void decode(const M& m, uint64_t n, uint64_t p, const int32_t* refmap, int32_t n_ref, Decoded* o) {
  o->rec.ref_new = o->rec.matched = o->rec.total = o->rec.flag_len = 0;
  o->qbeg = 0;
  o->qlen = 0;
  o->retained = 0;
  o->kind = kNone;
  uint64_t nx = 0;
  if (p > n || check(m, n, p, n_ref, &nx) != kOk) { o->kind = kCorrupt; return; }
  const uint64_t end = nx;
  const int32_t ref = (int32_t)ld32(m, p + 4), nref = (int32_t)ld32(m, p + 24);
  const uint32_t lrn = m[p + 12], ncig = ld16(m, p + 16), flag = ld16(m, p + 18), lseq = ld32(m, p + 20);
  const uint64_t qn = p + 4 + kFixed, cig = qn + lrn, qual = cig + 4ull * ncig + ((uint64_t)lseq + 1) / 2, aux = qual + lseq;
  const uint32_t qlen = lrn - 1;
  if (qlen && m[qn] == '@') return;  // line.startswith('@'): the reference skips it (:204)
  bool field = qlen > 0;
  for (uint32_t i = 0; i < qlen && field; ++i) field = graph(m[qn + i]);
  if (!field) { o->kind = kHost; return; }
  if (flag & 4) return;
  const int32_t row = refmap[ref + 1];
  if (row == -2) { o->kind = kHost; return; }
  if (ncig == 0) return;
  // a retained record from here on
  uint64_t matched = 0, total = 0;
  bool eq = false;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = ld32(m, cig + 4ull * i);
    const uint32_t op = v & 15u, len = v >> 4;
    if (op > 8) { o->kind = kCorrupt; return; }
    if (op == 7) eq = true;
    if (op == 0) matched += len;
    total += len;
  }
  if (ncig == 2 && (ld32(m, cig) & 15u) == 4 && (ld32(m, cig) >> 4) == lseq && (ld32(m, cig + 4) & 15u) == 3) {
    for (uint64_t t = aux; t < end;) {  // the long-read placeholder: the real CIGAR is in CG:B,I
      if (end - t >= 3 && m[t] == 'C' && m[t + 1] == 'G') { o->kind = kCorrupt; return; }
      if (!aux_skip(m, end, &t)) { o->kind = kCorrupt; return; }
    }
  }
  if (nref != -1 && nref != ref && refmap[nref + 1] == -2) { o->kind = kHost; return; }  // RNEXT: '=' / '*' / the name
  if (lseq && m[qual] != 0xff)
    for (uint64_t i = 0; i < lseq; ++i)
      if (m[qual + i] > 93) { o->kind = kHost; return; }  // QUAL byte + 33 beyond '~'
  uint32_t kind = kNone;
  if (row < 0) kind = kKey;
  else if (eq) kind = kValue;
  else if (aux == end) kind = kIndex;
  else {
    if (end - aux < 3) { o->kind = kCorrupt; return; }
    if (!graph(m[aux]) || !graph(m[aux + 1])) { o->kind = kHost; return; }
    uint64_t t = aux;
    if (!aux_skip(m, end, &t)) { o->kind = kCorrupt; return; }
    const uint32_t ty = m[aux + 2];
    const uint64_t v = aux + 3;
    switch (ty) {
      case 'c': case 'C': case 's': case 'S': case 'i': case 'I': break;  // ':i:' and a decimal
      case 'A': {
        const uint32_t c = m[v];
        if (!(c >= '0' && c <= '9')) {
          if (!graph(c)) { o->kind = kHost; return; }
          kind = kValue;
        }
        break;
      }
      case 'Z': case 'H': {
        uint64_t e = v;
        while (m[e] != 0 && !split_ws(m[e])) {  // (aux_skip found the NUL)
          if (m[e] >= 0x80) { o->kind = kHost; return; }
          ++e;
        }
        uint64_t d = v;
        if (d < e && (m[d] == '+' || m[d] == '-')) ++d;
        bool ok = d < e;
        for (; ok && d < e; ++d) ok = m[d] >= '0' && m[d] <= '9';
        if (!ok) kind = kValue;
        break;
      }
      case 'f': o->kind = kHost; return;
      default: kind = kValue; break;  // 'B': int('c,1,2')
    }
  }
  if (kind == kNone && total == 0) kind = kZeroDiv;
  if (kind == kNone && (lseq > MG_REC_MAX_SEQLEN || matched > 0xffffffffull || total > 0xffffffffull)) kind = kOverflow;
  if (kind != kNone) { o->kind = kind; return; }
  o->retained = 1;
  o->rec.ref_new = (uint32_t)row;
  o->rec.matched = (uint32_t)matched;
  o->rec.total = (uint32_t)total;
  o->rec.flag_len = (flag & MG_REC_FLAG_MASK) | (lseq << MG_REC_LEN_SHIFT);
  o->qbeg = qn;
  o->qlen = qlen;
}

// ---- reads (stages A / B) ----
constexpr uint32_t kFlagReverse = 0x10, kFlagNotRead = 0x900;  // (0x100 secondary | 0x800 supplementary)

MGB_HD bool seq_kept(uint32_t flag) { return (flag & kFlagNotRead) == 0; }

// code -> ASCII, and code -> the ASCII of its complement
MGB_HD uint8_t seq_ascii(uint32_t code) { return (uint8_t)"=ACMGRSVTWYHKDBN"[code & 15u]; }
MGB_HD uint8_t seq_ascii_comp(uint32_t code) { return (uint8_t)"=TGKCYSBAWRDMHVN"[code & 15u]; }

// Where the SEQ of the complete record at p (check() said kOk) lies: *seq = its first packed byte, *lseq, *flag.
template <class M>
MGB_HD void seq_span(const M& m, uint64_t p, uint64_t* seq, uint32_t* lseq, uint32_t* flag) {
  const uint32_t lrn = m[p + 12], ncig = ld16(m, p + 16);
  *flag = ld16(m, p + 18);
  *lseq = ld32(m, p + 20);
  *seq = p + 4 + kFixed + lrn + 4ull * ncig;
}

// The record's kept length (0 when it is not a read; *kept tells the two zeros apart).
template <class M>
MGB_HD uint32_t kept_len(const M& m, uint64_t p, uint32_t* kept) {
  const uint32_t flag = ld16(m, p + 18);
  *kept = seq_kept(flag) ? 1u : 0u;
  return *kept ? ld32(m, p + 20) : 0u;
}

// Base j (< lseq) of the read whose packed SEQ starts at seq: reverse = flag & 0x10.  One load, inside [seq, seq + (lseq + 1) / 2).
template <class M>
MGB_HD uint8_t seq_base(const M& m, uint64_t seq, uint32_t lseq, bool reverse, uint32_t j) {
  const uint32_t i = reverse ? lseq - 1u - j : j;
  const uint32_t code = (m[seq + (i >> 1)] >> ((i & 1u) ? 0 : 4)) & 15u;
  return reverse ? seq_ascii_comp(code) : seq_ascii(code);
}

}  // namespace mgb
