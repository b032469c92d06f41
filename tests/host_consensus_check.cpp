// host_consensus_check — the consensus part of mg_variants_core.h on the host, under the sanitizers (tests/test_consensus_host.py
// builds and runs it).
//
// The case file (little-endian): u32 nchars, then per character u32 n[4], u32 D, C, F, u32 iupac, u32 want (the character).
// Then u32 ntexts and per text u64 L, u32 width, u64 nbytes, L bytes (the sequence, no newline among them), nbytes bytes (its text as
// consensus.text_of writes it).  text_bytes() must give nbytes, and text_at() must be the exact inverse of the layout: byte i is a
// newline where the text has one, else it shows the next site — 0, 1, ... L - 1 in this order — and the text's byte is that site's.
// Then, by arithmetic only, one L above 2^32.  Prints what differs; exit status 1 when something did.
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
// exactly n bytes on the heap: a read behind them is the sanitizer's
static uint8_t* block(uint64_t n) {
  if (at + n > file.size()) { std::fprintf(stderr, "case file truncated\n"); std::exit(2); }
  uint8_t* m = static_cast<uint8_t*>(std::malloc(n ? n : 1));
  std::memcpy(m, file.data() + at, n);
  at += n;
  return m;
}

static int check_large() {
  int bad = 0;
  const uint32_t w = 60;
  const uint64_t L = (1ull << 32) + 12345, bytes = mgvar::text_bytes(L, w);
  if (bytes != L + (L + w - 1) / w || bytes != 4366562636ull) { std::printf("text_bytes(2^32 + 12345, 60) = %llu\n", (unsigned long long)bytes); ++bad; }
  const uint64_t sites[] = {0, 59, 60, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 59, L - 2, L - 1};
  for (uint64_t s : sites) {
    const uint64_t i = s + s / w;
    const mgvar::TextAt t = mgvar::text_at(i, w, L), u = mgvar::text_at(i, w);
    const mgvar::TextAt next = mgvar::text_at(i + 1, w, L);
    const bool closes = (s + 1) % w == 0 || s == L - 1;
    if (t.newline || t.site != s || u.newline || u.site != s || next.newline != closes || (!closes && next.site != s + 1)) {
      std::printf("L 2^32 + 12345, site %llu: byte %llu is site %llu (newline %d), the next a newline %d\n", (unsigned long long)s,
                  (unsigned long long)i, (unsigned long long)t.site, (int)t.newline, (int)next.newline);
      ++bad;
    }
  }
  if (!mgvar::text_at(bytes - 1, w, L).newline) { std::printf("the last byte of the large text is no newline\n"); ++bad; }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) { std::perror(argv[1]); return 2; }
  uint8_t buf[1 << 16];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) file.insert(file.end(), buf, buf + n);
  std::fclose(fh);
  int bad = 0;
  const uint32_t nchars = rd32();
  for (uint32_t i = 0; i < nchars; ++i) {
    uint32_t n[4];
    for (auto& x : n) x = rd32();
    const uint32_t D = rd32(), C = rd32(), F = rd32(), iupac = rd32(), want = rd32();
    const uint32_t got = mgvar::consensus_char(n, D, C, F, iupac != 0);
    if (got != want) {
      std::printf("character %u: [%u %u %u %u] (%u %u %u) iupac %u gives %c, expected %c\n", i, n[0], n[1], n[2], n[3], D, C, F, iupac,
                  (int)got, (int)want);
      ++bad;
    }
  }
  const uint32_t ntexts = rd32();
  for (uint32_t k = 0; k < ntexts; ++k) {
    const uint64_t L = rd64();
    const uint32_t width = rd32();
    const uint64_t nbytes = rd64();
    uint8_t* seq = block(L);
    uint8_t* text = block(nbytes);
    bool same = mgvar::text_bytes(L, width) == nbytes;
    uint64_t next_site = 0;
    for (uint64_t i = 0; same && i < nbytes; ++i) {
      const mgvar::TextAt t = mgvar::text_at(i, width, L);
      if (t.newline) {
        same = text[i] == '\n';
      } else {
        same = t.site == next_site && t.site < L && text[i] == seq[t.site] && text[i] != '\n';
        ++next_site;
      }
      // (without L: the same but for the newline behind a short last line, which stands where site L would)
      const mgvar::TextAt u = mgvar::text_at(i, width);
      if (same && i + 1 < nbytes) same = u.newline == t.newline && (u.newline || u.site == t.site);
      if (same && i + 1 == nbytes) same = u.newline || u.site == L;
    }
    same = same && next_site == (nbytes ? L : 0);
    std::free(seq);
    std::free(text);
    if (!same) {
      std::printf("text %u: L %llu, width %u, %llu bytes\n", k, (unsigned long long)L, width, (unsigned long long)nbytes);
      ++bad;
    }
  }
  bad += check_large();
  std::printf("%u characters, %u texts, %d differ\n", nchars, ntexts, bad);
  return bad ? 1 : 0;
}
