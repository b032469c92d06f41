// mg_refseq_core.h — what parsing a reference FASTA by RECORD into one code per site decides per byte, per line and per record
// (--ani, --vcf; metalign_amd/refseq.py is the definition): shared by the kernels of mg_refseq.hip and the host check.
//
//   is_white()       the bytes a sequence line is stripped of at both ends and a record's name ends at: space, tab, \r, \v, \f
//   classify_line()  a line without its '\n': a header (its first byte is '>') with the span of its name, or a sequence line with
//                    its stripped span.  Bytes inside a sequence line are kept
//   kind_of()        a record's kind from whether its name is a row, whether it is the FIRST record of that row, its bases and the
//                    row's length: loaded, foreign, mismatched, duplicate
//   parse_text()     the rules applied line by line to a whole file (the host check; the kernels apply them line-parallel)
//
// Codes are mgvar::code_of's.  Written so that the SAME code compiles for the host (tests/host_refdiff_check.cpp) and for gfx950.
// Memory is reached through an accessor (`m[i]` = byte i); no byte at or behind the end of a line is read.
#pragma once
#include <stdint.h>

#include "mg_variants_core.h"

namespace mgrs {

enum Kind : uint32_t { kLoaded = 0, kForeign = 1, kMismatched = 2, kDuplicate = 3 };
// (the counters of mg_refseq_stats: records, then one per kind in this order)

MGV_HD bool is_white(uint32_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

struct Line {
  bool head;
  uint64_t b, e;  // a header: its name; a sequence line: its stripped span
};

template <class M> MGV_HD Line classify_line(const M& m, uint64_t beg, uint64_t end) {
  Line l;
  l.head = beg < end && (uint8_t)m[beg] == '>';
  if (l.head) {
    l.b = l.e = beg + 1;
    while (l.e < end && !is_white((uint8_t)m[l.e])) ++l.e;
  } else {
    l.b = beg;
    l.e = end;
    while (l.e > l.b && is_white((uint8_t)m[l.e - 1])) --l.e;
    while (l.b < l.e && is_white((uint8_t)m[l.b])) ++l.b;
  }
  return l;
}

MGV_HD Kind kind_of(bool has_row, bool first_of_row, uint64_t nbases, uint64_t length) {
  if (!has_row) return kForeign;
  if (!first_of_row) return kDuplicate;
  return nbases == length ? kLoaded : kMismatched;
}

// The text m[0 .. n) record by record.  row_of(b, e): the row of the name m[b .. e), or -1 (an empty name: -1).  off[row]: where the
// row's codes go in `codes` (out[i] = byte); seen[row], loaded[row]: zeroed by the caller; stats[5]: zeroed by the caller.
template <class M, class RowOf, class Out>
MGV_HD void parse_text(const M& m, uint64_t n, const RowOf& row_of, const uint64_t* lengths, const uint64_t* off, Out& codes,
                       uint8_t* seen, uint8_t* loaded, uint64_t stats[5]) {
  bool open = false;
  int64_t row = -1;
  uint64_t body = 0, nbases = 0;  // the open record: where its lines start, its bases so far
  uint64_t lb = 0;
  for (;;) {
    // the line [lb, le); behind the last line: one more turn that only closes the open record
    const bool done = lb > n;
    uint64_t le = lb;
    Line l{true, 0, 0};
    if (!done) {
      while (le < n && (uint8_t)m[le] != '\n') ++le;
      l = classify_line(m, lb, le);
    }
    if (l.head) {
      if (open) {
        const bool has_row = row >= 0, first = has_row && !seen[row];
        const Kind k = kind_of(has_row, first, nbases, has_row ? lengths[row] : 0);
        ++stats[0];
        ++stats[1 + k];
        if (first) seen[row] = 1;
        if (k == kLoaded) {
          loaded[row] = 1;
          uint64_t at = off[row];
          const uint64_t stop = lb < n ? lb : n;  // (the record's lines again: [body, stop) holds whole lines, none of them a header)
          for (uint64_t p = body; p < stop;) {
            uint64_t q = p;
            while (q < stop && (uint8_t)m[q] != '\n') ++q;
            const Line s = classify_line(m, p, q);
            for (uint64_t i = s.b; i < s.e; ++i) codes[at++] = (uint8_t)mgvar::code_of((uint8_t)m[i]);
            p = q + 1;
          }
        }
      }
      if (done) return;
      open = true;
      row = l.e > l.b ? row_of(l.b, l.e) : -1;
      body = le < n ? le + 1 : n;
      nbases = 0;
    } else if (open) {
      nbases += l.e - l.b;
    }
    lb = le + 1;
  }
}

}  // namespace mgrs
