// host_align_check.cpp — mg_align_core.h on the host (tests/test_align_host.py builds this with the sanitizers and compares its
// output with metalign_amd/align.py).  The case file, little endian:
//   u32 nseq, then per sequence: u32 k, u32 w, u32 n, n code bytes       -> "S <i> <number of minimizers>", then "m <p> <key> <strand>"
//   u32 nscan, then per scan: u32 P, u32 n, n column bytes (0 outside, 1 adds 1, 2 subtracts P)
//                                                                        -> "C <i> <score> <b> <e> <nm>"
//   u32 nsel, then per selection: u32 max_secondary, u32 sec_pct, u32 n, n x (u32 a, strand, pos0, span, score), in order
//                                                                        -> "K <i> <kept indices ...>"
// Every byte a rule reads lies inside its sequence: the sequences are heap blocks of exactly their size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_align_core.h"

namespace {

std::vector<uint8_t> g_file;
size_t g_at = 0;

uint32_t u32() {
  uint32_t v;
  if (g_at + 4 > g_file.size()) {
    fprintf(stderr, "case file too short\n");
    exit(2);
  }
  memcpy(&v, g_file.data() + g_at, 4);
  g_at += 4;
  return v;
}

struct Codes {
  const uint8_t* p;
  uint64_t n;
  uint32_t operator()(uint64_t i) const {
    if (i >= n) {
      fprintf(stderr, "read of base %llu of %llu\n", (unsigned long long)i, (unsigned long long)n);
      exit(3);
    }
    return p[i];
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  g_file.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (fread(g_file.data(), 1, g_file.size(), f) != g_file.size()) return 2;
  fclose(f);

  const uint32_t nseq = u32();
  for (uint32_t i = 0; i < nseq; ++i) {
    const uint32_t k = u32(), w = u32(), n = u32();
    uint8_t* codes = new uint8_t[n ? n : 1];  // (its own block: a read behind it is the sanitizer's)
    memcpy(codes, g_file.data() + g_at, n);
    g_at += n;
    std::vector<uint64_t> pos;
    std::vector<mga::Key> keys;
    if (n >= k) {
      for (uint64_t p = 0; p + k <= n; ++p) {
        mga::Key key;
        if (mga::minimizer_at(Codes{codes, n}, n, p, k, w, &key)) {
          pos.push_back(p);
          keys.push_back(key);
        }
      }
    }
    printf("S %u %zu\n", i, pos.size());
    for (size_t j = 0; j < pos.size(); ++j)
      printf("m %llu %llu %u\n", (unsigned long long)pos[j], (unsigned long long)keys[j].key, keys[j].strand);
    delete[] codes;
  }

  const uint32_t nscan = u32();
  for (uint32_t i = 0; i < nscan; ++i) {
    const uint32_t P = u32(), n = u32();
    mga::Scan s;
    for (uint32_t j = 0; j < n; ++j) {
      const uint8_t c = g_file[g_at + j];
      mga::step(s, (int32_t)j, c != 0, c == 1, (int32_t)P);
    }
    g_at += n;
    printf("C %u %d %d %d %u\n", i, s.best, s.b, s.e, mga::nm_of((uint32_t)(s.e - s.b), (uint32_t)s.best, P));
  }

  const uint32_t nsel = u32();
  for (uint32_t i = 0; i < nsel; ++i) {
    const uint32_t max_secondary = u32(), sec_pct = u32(), n = u32();
    struct Al { uint32_t a, strand, pos0, span, score; };
    std::vector<Al> kept;
    printf("K %u", i);
    for (uint32_t j = 0; j < n; ++j) {
      Al al{u32(), u32(), u32(), u32(), u32()};
      if (kept.size() >= 1 + (size_t)max_secondary) continue;
      bool ok = kept.empty() || mga::secondary_ok(al.score, kept[0].score, sec_pct);
      for (const Al& x : kept)
        ok = ok && !mga::overlaps(x.a, x.strand, x.pos0, x.pos0 + x.span, al.a, al.strand, al.pos0, al.pos0 + al.span);
      if (ok) {
        kept.push_back(al);
        printf(" %u", j);
      }
    }
    printf("\n");
  }
  printf("%u sequences, %u scans, %u selections\n", nseq, nscan, nsel);
  return 0;
}
