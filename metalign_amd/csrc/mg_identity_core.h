// mg_identity_core.h — the arithmetic of an alignment's edit distance and aligned columns (--identity; metalign_amd/identity.py is
// the definition): what the tokenisers' edit kernels (k_sam_edit, k_bam_edit in mg_ingest.hip) and the identity kernel
// (mg_identity.hip) decide per record.
//
//   NmScan         the search for the first field that starts with `NM:i:` among the fields of line.strip().split() from the twelfth
//                  on, as a machine fed one byte at a time: fields are maximal runs of bytes that are not white space, the first one
//                  with that prefix ends the search, and its value is usable when it is [+-]?[0-9]+ with 0 <= value <= 2^32 - 2
//                  (digits saturate, they never wrap).  Everything else — no such field, an empty or malformed value, a negative
//                  one, one too large — is kNone.
//   cigar_cols()   the alignment columns of a CIGAR string: the lengths of its M, I, D and X ops, at most 2^32 - 1
//   bam_cols()     the same over a BAM record's packed ops: codes 0 (M), 1 (I), 2 (D), 8 (X)
//   edit_of_line() a retained SAM line: cig = the start of its CIGAR field, tags = the start of its twelfth field, end = its end;
//                  fields that are not NM:i: are stepped over by the caller's skip (a byte at a time here, 8-byte loads on the device)
//   edit_of_bam()  a BAM record, held to its SAM rendering (metalign_amd/bam.py: render): every aux field is fed to the machine as
//                  it renders — TAG:i:<decimal> for the types c C s S i I, TAG:A:<byte>, TAG:Z:<bytes> / TAG:H:<bytes>, and TAG:f: /
//                  TAG:B: with a value that holds no white space — with a TAB between fields.  So an `NM` of another type is not
//                  NM:i:, and a Z / H value or an A byte with white space inside cuts its field in pieces, each judged like any
//                  other field.  A malformed aux field ends the walk with kNone; no byte at or behind the record's end is read.
//   bin_of()       (cols - e) * 1000 / cols, e = min(nm, cols): 0 .. 1000
//
// Written so that the SAME code compiles for the host (tests/host_identity_check.cpp) and for gfx950.  Memory is reached through
// an accessor (`m[i]` = byte i).
#pragma once
#include <stdint.h>

#include "../../include/metalign_hip.h"
#include "mg_bam_core.h"
#include "mg_coverage_core.h"

namespace mgi {

constexpr uint32_t kNone = 0xffffffffu;          // no usable NM:i:
constexpr uint64_t kMaxNm = 0xfffffffeull, kMaxCols = 0xffffffffull;
constexpr uint32_t kBins = 1001;

struct NmScan {
  // st: 0 between fields; 1 .. 4 that many bytes of "NM:i:" matched from a field's start; 5 inside the value; 6 inside a field
  // that is not it; 7 the search is over
  uint32_t st = 0, vlen = 0, ndig = 0;
  bool neg = false, bad = false;
  uint64_t v = 0;

  MGV_HD bool done() const { return st == 7; }
  MGV_HD bool in_value() const { return st == 5; }
  MGV_HD void feed(uint32_t c) {
    if (st == 7) return;
    if (mgv::is_ws(c)) {
      st = st == 5 ? 7u : 0u;
      return;
    }
    switch (st) {
      case 0: st = c == 'N' ? 1u : 6u; break;
      case 1: st = c == 'M' ? 2u : 6u; break;
      case 2: st = c == ':' ? 3u : 6u; break;
      case 3: st = c == 'i' ? 4u : 6u; break;
      case 4: st = c == ':' ? 5u : 6u; break;
      case 5:
        if (vlen == 0 && (c == '+' || c == '-')) {
          neg = c == '-';
        } else if (c >= '0' && c <= '9') {
          v = v * 10 + (c - '0');
          if (v > kMaxNm) v = kMaxNm + 1;  // (stays there: too large)
          ++ndig;
        } else {
          bad = true;
        }
        ++vlen;
        break;
      default: break;
    }
  }
  // the text is over: a value that was being read ends here
  MGV_HD uint32_t result() const {
    if (st != 5 && st != 7) return kNone;
    if (bad || ndig == 0 || v > kMaxNm || (neg && v != 0)) return kNone;
    return (uint32_t)v;
  }
};

template <class M> MGV_HD uint32_t cigar_cols(const M& m, uint64_t b, uint64_t e) {
  uint64_t cols = 0, cur = 0;
  for (uint64_t p = b; p < e; ++p) {
    const uint32_t c = m[p];
    if (mgv::is_alpha(c)) {
      if (c == 'M' || c == 'I' || c == 'D' || c == 'X') cols += cur;
      if (cols > kMaxCols) cols = kMaxCols;
      cur = 0;
    } else if (c >= '0' && c <= '9') {
      cur = cur * 10 + (c - '0');
      if (cur > kMaxCols) cur = kMaxCols;
    }
  }
  return (uint32_t)cols;
}

template <class M> MGV_HD uint32_t bam_cols(const M& m, uint64_t cig, uint32_t ncig) {
  uint64_t cols = 0;
  for (uint32_t i = 0; i < ncig; ++i) {
    const uint32_t v = mgb::ld32(m, cig + 4ull * i);
    const uint32_t op = v & 15u;
    if (op == 0 || op == 1 || op == 2 || op == 8) cols += v >> 4;
  }
  return (uint32_t)(cols > kMaxCols ? kMaxCols : cols);
}

// skip(m, p, end): the first white-space byte in [p, end), or end.  ByteSkip reads a byte at a time; the device passes the parser's
// 8-byte loads (mg_ingest.hip: scan_to_ws).
struct ByteSkip {
  template <class M> MGV_HD uint64_t operator()(const M& m, uint64_t p, uint64_t end) const {
    while (p < end && !mgv::is_ws(m[p])) ++p;
    return p;
  }
};

// nm of the fields of [p, end): a field that does not start with NM:i: is skipped, the first one that does ends the search and
// its value — the rest of the field — goes through the machine
template <class M, class Skip> MGV_HD uint32_t nm_of_text(const M& m, uint64_t p, uint64_t end, const Skip& skip) {
  while (p < end) {
    while (p < end && mgv::is_ws(m[p])) ++p;
    if (p >= end) break;
    if (end - p >= 5 && m[p] == 'N' && m[p + 1] == 'M' && m[p + 2] == ':' && m[p + 3] == 'i' && m[p + 4] == ':') {
      NmScan s;
      s.st = 5;  // (inside the value)
      for (p += 5; p < end && !s.done(); ++p) s.feed(m[p]);
      return s.result();
    }
    p = skip(m, p, end);
  }
  return kNone;
}

template <class M, class Skip> MGV_HD mg_aln_edit edit_of_line(const M& m, uint64_t cig, uint64_t tags, uint64_t end, const Skip& skip) {
  mg_aln_edit ed;
  ed.cols = cigar_cols(m, cig, skip(m, cig, end));
  ed.nm = nm_of_text(m, tags, end, skip);
  return ed;
}

// The BAM record whose QNAME starts at qn (the record at qn - 36; decode() has judged it complete and retained it).
template <class M> MGV_HD mg_aln_edit edit_of_bam(const M& m, uint64_t qn) {
  mg_aln_edit ed;
  const uint64_t p = qn - 36;
  const uint64_t end = p + 4 + (uint64_t)mgb::ld32(m, p);
  const uint32_t lrn = m[p + 12], ncig = mgb::ld16(m, p + 16), lseq = mgb::ld32(m, p + 20);
  const uint64_t cig = qn + lrn, aux = cig + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + lseq;
  ed.cols = bam_cols(m, cig, ncig);
  ed.nm = kNone;
  NmScan s;
  uint64_t t = aux;
  while (t < end && !s.done()) {
    uint64_t nx = t;
    if (!mgb::aux_skip(m, end, &nx)) return ed;  // malformed: the walk ends, nm stays kNone
    const uint32_t ty = m[t + 2];
    s.feed(m[t]);
    s.feed(m[t + 1]);
    s.feed(':');
    const uint64_t v = t + 3;
    switch (ty) {
      case 'c': case 'C': case 's': case 'S': case 'i': case 'I': {
        s.feed('i');
        s.feed(':');
        if (s.in_value()) {  // (in any other state the digits change nothing)
          int64_t x;
          switch (ty) {
            case 'c': x = (int8_t)m[v]; break;
            case 'C': x = m[v]; break;
            case 's': x = (int16_t)mgb::ld16(m, v); break;
            case 'S': x = mgb::ld16(m, v); break;
            case 'i': x = (int32_t)mgb::ld32(m, v); break;
            default: x = mgb::ld32(m, v); break;
          }
          if (x < 0) { s.feed('-'); x = -x; }
          uint32_t dig[10];
          int nd = 0;
          do { dig[nd++] = (uint32_t)(x % 10); x /= 10; } while (x);
          while (nd) s.feed('0' + dig[--nd]);
        }
        break;
      }
      case 'A':
        s.feed('A');
        s.feed(':');
        s.feed(m[v]);
        break;
      case 'Z': case 'H':
        s.feed(ty);
        s.feed(':');
        for (uint64_t q = v; q + 1 < nx && !s.done(); ++q) s.feed(m[q]);  // (nx - 1 is the NUL)
        break;
      default:  // 'f', 'B': a value without white space
        s.feed(ty);
        s.feed(':');
        s.feed('x');
        break;
    }
    s.feed('\t');
    t = nx;
  }
  ed.nm = s.result();
  return ed;
}

// A scored alignment's edits and bin: cols > 0, nm != kNone.
MGV_HD uint32_t edits_of(uint32_t nm, uint32_t cols) { return nm < cols ? nm : cols; }
MGV_HD uint32_t bin_of(uint32_t e, uint32_t cols) { return (uint32_t)(((uint64_t)(cols - e) * 1000ull) / cols); }

}  // namespace mgi
