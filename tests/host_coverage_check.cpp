// The placement arithmetic of --coverage (metalign_amd/csrc/mg_coverage_core.h) compiled for the HOST, through an accessor that
// refuses any byte outside the line / record it is given.
// Input, five sections, each a u32 count and then per item:
//   SAM lines     u32 length + bytes                              -> "L pos0 span"
//   BAM records   u32 length + bytes (block_size first)           -> "B pos0 span"
//   intervals     u64 begin, u64 end                              -> "I w0 m0 w1 m1" and "W mask..." for up to 4 words from w0
//   clips         u32 pos0, u32 span, u64 L                       -> "C length"
//   counts        u32 matched, u32 total, u32 flag, f64 pct_id    -> "K 0|1"
// Driven by tests/test_coverage_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_coverage_core.h"

struct Checked {
  const unsigned char* p;
  uint64_t beg, end;
  unsigned char operator[](uint64_t i) const {
    if (i < beg || i >= end) { printf("load outside the item at %llu\n", (unsigned long long)i); exit(2); }
    return p[i];
  }
};

static std::vector<unsigned char> buf;
static uint64_t at = 0;
template <class T> static T take() {
  T v;
  if (at + sizeof(T) > buf.size()) { printf("short input\n"); exit(3); }
  memcpy(&v, buf.data() + at, sizeof(T));
  at += sizeof(T);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    const uint32_t len = take<uint32_t>();
    const Checked m{buf.data(), at, at + len};
    const mg_aln_place pl = mgv::place_of_line(m, at, at + len);
    printf("L %u %u\n", pl.pos0, pl.span);
    at += len;
  }
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    const uint32_t len = take<uint32_t>();
    const Checked m{buf.data(), at, at + len};
    const mg_aln_place pl = mgv::place_of_bam(m, at + 36);
    printf("B %u %u\n", pl.pos0, pl.span);
    at += len;
  }
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    const uint64_t b = take<uint64_t>(), e = take<uint64_t>();
    uint64_t w0, w1;
    uint32_t m0, m1;
    mgv::interval(b, e, &w0, &m0, &w1, &m1);
    printf("I %llu %u %llu %u\nW", (unsigned long long)w0, m0, (unsigned long long)w1, m1);
    for (uint64_t w = w0; w <= w1 && w < w0 + 4; ++w) printf(" %u", mgv::word_mask(w, w0, m0, w1, m1));
    printf("\n");
  }
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    const uint32_t pos0 = take<uint32_t>(), span = take<uint32_t>();
    const uint64_t L = take<uint64_t>();
    printf("C %llu\n", (unsigned long long)mgv::clipped(pos0, span, L));
  }
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    mg_aln_rec r;
    r.ref_new = 0;
    r.matched = take<uint32_t>();
    r.total = take<uint32_t>();
    r.flag_len = take<uint32_t>();
    const double pct = take<double>();
    printf("K %d\n", mgv::counts(r, pct) ? 1 : 0);
  }
  return 0;
}
