// Host check of mg_refseq_core.h (the reference FASTA by record) and of mgvar::diff_of (mg_variants_core.h), under the sanitizers:
// tests/test_refseq_host.py and tests/test_refdiff_host.py write the cases with what metalign_amd/refseq.py and refdiff.py say.
//
//   u32 ntexts, then per text:  u32 nbytes, u32 nacc, u64 lengths[nacc], per row (u32 n, its name), the text,
//                               u64 stats[5], u8 loaded[nacc], u8 codes[sum lengths] (0xff in the rows that are not loaded)
//   u32 nsites, then per site:  u32 n4[4], r, D, C, F, want (bit 0 compared, 1 ref_other, 2 con_sub, 3 pop_sub, 4 emitted)
//
// Every text lies in a heap block of exactly its size, so a read at or behind its end is an error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../metalign_amd/csrc/mg_refseq_core.h"

static std::vector<uint8_t> blob;
static size_t at = 0;

template <class T> static T take() {
  T v;
  if (at + sizeof(T) > blob.size()) { fprintf(stderr, "short case file\n"); exit(2); }
  memcpy(&v, blob.data() + at, sizeof(T));
  at += sizeof(T);
  return v;
}

static std::vector<uint8_t> take_bytes(size_t n) {
  if (at + n > blob.size()) { fprintf(stderr, "short case file\n"); exit(2); }
  std::vector<uint8_t> v(blob.begin() + at, blob.begin() + at + n);
  at += n;
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  unsigned differ = 0;
  const uint32_t ntexts = take<uint32_t>();
  for (uint32_t t = 0; t < ntexts; ++t) {
    const uint32_t nbytes = take<uint32_t>(), nacc = take<uint32_t>();
    std::vector<uint64_t> lengths(nacc), off(nacc + 1, 0);
    for (uint32_t a = 0; a < nacc; ++a) {
      lengths[a] = take<uint64_t>();
      off[a + 1] = off[a] + lengths[a];
    }
    std::map<std::string, int64_t> rows;
    for (uint32_t a = 0; a < nacc; ++a) {
      const uint32_t len = take<uint32_t>();
      const std::vector<uint8_t> name = take_bytes(len);
      rows[std::string(name.begin(), name.end())] = a;
    }
    const std::vector<uint8_t> text_in = take_bytes(nbytes);
    uint8_t* exact = nbytes ? new uint8_t[nbytes] : nullptr;  // (exactly the text: the sanitizer sees a byte too many)
    if (nbytes) memcpy(exact, text_in.data(), nbytes);
    uint64_t want_stats[5];
    for (int i = 0; i < 5; ++i) want_stats[i] = take<uint64_t>();
    const std::vector<uint8_t> want_loaded = take_bytes(nacc), want_codes = take_bytes(off[nacc]);
    std::vector<uint8_t> codes(off[nacc] + 1, 0xff), seen(nacc + 1, 0), loaded(nacc + 1, 0);
    uint64_t stats[5] = {0, 0, 0, 0, 0};
    const uint8_t* m = exact;
    auto row_of = [&](uint64_t b, uint64_t e) -> int64_t {
      const auto it = rows.find(std::string(m + b, m + e));
      return it == rows.end() ? -1 : it->second;
    };
    mgrs::parse_text(m, (uint64_t)nbytes, row_of, lengths.data(), off.data(), codes, seen.data(), loaded.data(), stats);
    bool bad = memcmp(stats, want_stats, sizeof stats) != 0 || memcmp(loaded.data(), want_loaded.data(), nacc) != 0 ||
               memcmp(codes.data(), want_codes.data(), off[nacc]) != 0 || codes[off[nacc]] != 0xff;
    if (bad) {
      ++differ;
      printf("text %u differs: stats %llu %llu %llu %llu %llu\n", t, (unsigned long long)stats[0], (unsigned long long)stats[1],
             (unsigned long long)stats[2], (unsigned long long)stats[3], (unsigned long long)stats[4]);
    }
    delete[] exact;
  }
  const uint32_t nsites = take<uint32_t>();
  for (uint32_t s = 0; s < nsites; ++s) {
    uint32_t v[9];
    for (int i = 0; i < 9; ++i) v[i] = take<uint32_t>();
    const mgvar::Diff d = mgvar::diff_of(v, v[4], v[5], v[6], v[7]);
    const uint32_t got = (d.compared ? 1u : 0u) | (d.ref_other ? 2u : 0u) | (d.con_sub ? 4u : 0u) | (d.pop_sub ? 8u : 0u) | (d.emitted ? 16u : 0u);
    if (got != v[8]) {
      ++differ;
      printf("site %u differs: got %u, want %u\n", s, got, v[8]);
    }
  }
  printf("%u texts, %u sites, %u differ\n", ntexts, nsites, differ);
  return differ ? 1 : 0;
}
