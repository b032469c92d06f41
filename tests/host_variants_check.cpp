// host_variants_check — mg_variants_core.h on the host, under the sanitizers (tests/test_variants_host.py builds and runs it).
//
// The case file (little-endian): u32 ncases, then per case
//   u32 kind      0: a SAM line, a .. b = its CIGAR field, c .. d = its SEQ field (offsets into the line)
//                 1: a BAM record (block_size first), a = the offset of its QNAME (36); b, c, d unused
//   u32 len, u32 a, u32 b, u32 c, u32 d, u32 want_span, want_span bytes (the expected codes, one per byte), then len bytes.
// then u32 nsites and per site u32 n[4], u32 D, C, F, u32 callable, major, variant mask, u64 pairs, u64 discordant.
// Every case's bytes are copied into a heap block of exactly len bytes, and the packed codes are written into one of exactly
// (span + 1) / 2 bytes, so that a read or write at or behind an end is an error the sanitizer reports.  Prints every case that
// differs; exit status 1 when one did.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_variants_core.h"

static std::vector<uint8_t> file;
static size_t at = 0;

static uint32_t rd32() {
  if (at + 4 > file.size()) { std::fprintf(stderr, "case file truncated\n"); std::exit(2); }
  uint32_t x;
  std::memcpy(&x, file.data() + at, 4);
  at += 4;
  return x;
}
static uint64_t rd64() {
  const uint64_t lo = rd32();
  return lo | ((uint64_t)rd32() << 32);
}

struct VecSink {
  std::vector<uint8_t> codes;
  void put(uint32_t c) { codes.push_back((uint8_t)c); }
};

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror(argv[1]); return 2; }
  uint8_t buf[1 << 16];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) file.insert(file.end(), buf, buf + n);
  std::fclose(fh);
  const uint32_t ncases = rd32();
  int bad = 0;
  for (uint32_t i = 0; i < ncases; ++i) {
    const uint32_t kind = rd32(), len = rd32(), a = rd32(), b = rd32(), c = rd32(), d = rd32(), want_span = rd32();
    if (at + want_span + len > file.size()) { std::fprintf(stderr, "case file truncated\n"); return 2; }
    const std::vector<uint8_t> want(file.begin() + at, file.begin() + at + want_span);
    at += want_span;
    uint8_t* m = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memcpy(m, file.data() + at, len);
    at += len;
    const uint8_t* cm = m;
    const uint32_t span = kind == 0 ? mgvar::sam_pile_span(cm, a, b, c, d) : mgvar::bam_pile_span(cm, a);
    VecSink sink;
    uint8_t* packed = static_cast<uint8_t*>(std::malloc(span ? (span + 1) / 2 : 1));
    if (span) {
      mgvar::NibblePacker<uint8_t*> pk(packed, 0);
      if (kind == 0) {
        mgvar::sam_pile_walk(cm, a, b, c, sink);
        mgvar::sam_pile_walk(cm, a, b, c, pk);
      } else {
        mgvar::bam_pile_walk(cm, a, sink);
        mgvar::bam_pile_walk(cm, a, pk);
      }
      pk.flush();
    }
    bool same = span == want_span && sink.codes == want;
    for (uint32_t j = 0; same && j < span; ++j) same = mgvar::code_at(packed, 0, j) == want[j];
    if (same && (span & 1u)) same = (packed[span / 2] >> 4) == 0;  // (the unused high nibble of an odd span)
    std::free(packed);
    std::free(m);
    if (!same) {
      std::printf("case %u (kind %u): span %u, expected %u; codes", i, kind, span, want_span);
      for (uint8_t x : sink.codes) std::printf(" %u", x);
      std::printf("\n");
      ++bad;
    }
  }
  const uint32_t nsites = rd32();
  for (uint32_t i = 0; i < nsites; ++i) {
    uint32_t n[4];
    for (auto& x : n) x = rd32();
    const uint32_t D = rd32(), C = rd32(), F = rd32(), w_call = rd32(), w_major = rd32(), w_mask = rd32();
    const uint64_t w_pairs = rd64(), w_disc = rd64();
    const mgvar::Site s = mgvar::site_of(n, D, C, F);
    if ((uint32_t)s.callable_ != w_call || s.major != w_major || s.variants != w_mask || s.pairs != w_pairs || s.discordant != w_disc ||
        s.polymorphic != (w_mask != 0)) {
      std::printf("site %u: callable %d major %u mask %u pairs %llu discordant %llu\n", i, (int)s.callable_, s.major, s.variants,
                  (unsigned long long)s.pairs, (unsigned long long)s.discordant);
      ++bad;
    }
  }
  std::printf("%u cases, %u sites, %d differ\n", ncases, nsites, bad);
  return bad ? 1 : 0;
}
