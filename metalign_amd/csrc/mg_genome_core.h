// mg_genome_core.h — what parsing an organism FASTA file into ONE genome (mg_genome.hip) decides per line.
//
// The definition is metalign_amd/build_db.py (genome_bases): a line that starts with '>' opens a record; every other line after the
// file's first header is stripped of white space at both ends and appended; lines in front of the first header are dropped; the
// records of a file are joined by exactly one 'N' — every header line but the file's first emits one, an empty record's too.
// Case and non-ACGT bytes are kept.
//
//   is_space()        the white space stripped from a line: the set of mg_ingest.hip (format 2), byte for byte
//   stripped_span()   [beg, end) of a line without the white space at its ends
//   undecided_byte()  a byte on which Python's text mode and these byte rules part: a '\r' that no '\n' follows (text mode ends a
//                     line there), 0x1c-0x1f (str.strip() removes them), >= 0x80 (the locale's decoder).  A file that holds one
//                     is NOT decided here: the caller parses it with genome_bases
//   classify_line()   header or not, and the stripped span
//   nameless_header() a header line that is '>' and white space only, with at least one byte behind the '>' (its '\n' counts):
//                     formats.read_sequences RAISES on it (the name is line[1:].split()[0]), so nothing is defined — such a file
//                     is left undecided as well, and the caller's genome_bases raises as the host path does
//   emitted()         the bytes a line adds to its genome, given how many header lines of the file stand in front of it
//   genome_file()     the rules applied line by line to a whole file (the host check; the kernels apply them line-parallel)
//
// Written so that the SAME code compiles for the host (tests/host_genome_check.cpp) and for gfx950.  Bytes are read one at a time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MGG_HD __host__ __device__ inline
#else
#define MGG_HD inline
#endif

namespace mgg {

MGG_HD bool is_space(uint8_t ch) {
  return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\v' || ch == '\f';
}

// m[beg .. end): a line without its '\n'.  M is anything with operator[] (a pointer; the host test's checked array).
template <class M> MGG_HD void stripped_span(const M& m, uint64_t& beg, uint64_t& end) {
  while (end > beg && is_space((uint8_t)m[end - 1])) --end;
  while (beg < end && is_space((uint8_t)m[beg])) ++beg;
}

// ch with the byte behind it in the same file (has_next = there is one)
MGG_HD bool undecided_byte(uint8_t ch, bool has_next, uint8_t next) {
  return ch >= 0x80 || (ch >= 0x1c && ch <= 0x1f) || (ch == '\r' && !(has_next && next == '\n'));
}

// the line m[beg .. end): true = a header; [*sb, *se) = its stripped span
template <class M> MGG_HD bool classify_line(const M& m, uint64_t beg, uint64_t end, uint64_t* sb, uint64_t* se) {
  const bool head = beg < end && (uint8_t)m[beg] == '>';
  *sb = beg;
  *se = end;
  stripped_span(m, *sb, *se);
  return head;
}

// raw_len: the line's bytes without its '\n'; has_newline: it ends in one (a file's last line need not)
MGG_HD bool nameless_header(bool head, uint64_t stripped_len, uint64_t raw_len, bool has_newline) {
  return head && stripped_len == 1 && (raw_len > 1 || has_newline);
}

// headers_before: the header lines of the same file in front of this line.  A header emits the joining 'N', a sequence line its
// stripped bytes (a line of 2^32 bytes or more is not one this parser is given: the caller's pieces are smaller).
MGG_HD uint32_t emitted(bool head, uint64_t stripped_len, uint64_t headers_before) {
  if (headers_before == 0) return 0;
  return head ? 1u : (uint32_t)stripped_len;
}

// The file m[beg .. end) line by line: emit(byte) for every byte of its genome.  false = undecided (what was emitted is void).
template <class M, class Emit> MGG_HD bool genome_file(const M& m, uint64_t beg, uint64_t end, Emit emit) {
  for (uint64_t p = beg; p < end; ++p)
    if (undecided_byte((uint8_t)m[p], p + 1 < end, p + 1 < end ? (uint8_t)m[p + 1] : 0)) return false;
  uint64_t headers = 0;
  uint64_t lb = beg;
  while (lb < end) {
    uint64_t le = lb;
    while (le < end && (uint8_t)m[le] != '\n') ++le;
    uint64_t sb, se;
    const bool head = classify_line(m, lb, le, &sb, &se);
    if (nameless_header(head, se - sb, le - lb, le < end)) return false;
    const uint32_t n = emitted(head, se - sb, headers);
    if (head) { if (n) emit((uint8_t)'N'); ++headers; }
    else for (uint32_t i = 0; i < n; ++i) emit((uint8_t)m[sb + i]);
    lb = le + 1;
  }
  return true;
}

}  // namespace mgg
