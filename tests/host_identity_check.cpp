// host_identity_check — mg_identity_core.h on the host, under the sanitizers (tests/test_identity_host.py builds and runs it).
//
// The case file (little-endian): u32 ncases, then per case
//   u32 kind      0: a SAM line, a = the offset of its CIGAR field, b = the offset of its twelfth field (= len when it has none)
//                 1: a BAM record (block_size first), a = the offset of its QNAME (36), b unused
//   u32 len, u32 a, u32 b, u32 want_nm, u32 want_cols, then len bytes.
// Every case's bytes are copied into a heap block of exactly len bytes, so that a read at or behind the end is an error the
// sanitizer reports.  Prints every case that differs; exit status 1 when one did.  Also checks bin_of / edits_of on a few values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_identity_core.h"

static uint32_t rd32(const std::vector<uint8_t>& v, size_t& at) {
  if (at + 4 > v.size()) { std::fprintf(stderr, "case file truncated\n"); std::exit(2); }
  uint32_t x;
  std::memcpy(&x, v.data() + at, 4);
  at += 4;
  return x;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror(argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t buf[1 << 16];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) file.insert(file.end(), buf, buf + n);
  std::fclose(fh);
  size_t at = 0;
  const uint32_t ncases = rd32(file, at);
  int bad = 0;
  for (uint32_t i = 0; i < ncases; ++i) {
    const uint32_t kind = rd32(file, at), len = rd32(file, at), a = rd32(file, at), b = rd32(file, at);
    const uint32_t want_nm = rd32(file, at), want_cols = rd32(file, at);
    if (at + len > file.size()) { std::fprintf(stderr, "case file truncated\n"); return 2; }
    uint8_t* m = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(m, file.data() + at, len);
    at += len;
    const uint8_t* cm = m;
    const mg_aln_edit got = kind == 0 ? mgi::edit_of_line(cm, a, b, len, mgi::ByteSkip()) : mgi::edit_of_bam(cm, a);
    std::free(m);
    if (got.nm != want_nm || got.cols != want_cols) {
      std::printf("case %u (kind %u): nm %u cols %u, expected nm %u cols %u\n", i, kind, got.nm, got.cols, want_nm, want_cols);
      ++bad;
    }
  }
  // the per-alignment arithmetic
  struct { uint32_t nm, cols, e, bin; } arith[] = {{0, 10, 0, 1000}, {1, 10, 1, 900}, {25, 10, 10, 0}, {9, 20, 9, 550}, {7, 100, 7, 930},
                                                   {1, 0xffffffffu, 1, 999}, {0xfffffffeu, 0xffffffffu, 0xfffffffeu, 0}, {1, 3, 1, 666}};
  for (const auto& c : arith) {
    const uint32_t e = mgi::edits_of(c.nm, c.cols), bin = mgi::bin_of(e, c.cols);
    if (e != c.e || bin != c.bin) {
      std::printf("arith nm %u cols %u: e %u bin %u, expected %u %u\n", c.nm, c.cols, e, bin, c.e, c.bin);
      ++bad;
    }
  }
  std::printf("%u cases, %d differ\n", ncases, bad);
  return bad ? 1 : 0;
}
