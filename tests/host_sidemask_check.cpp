// Host check of metalign_amd/csrc/mg_sidemask_core.h (tests/test_side_reads_host.py builds it with the sanitizers): the per-record
// decision of --side_reads unique, with the read ordinals from a scalar restatement of the device's three phases (NEW bits per tile,
// the exclusive scan of the tiles in 64 bits, the prefix inside the tile).
//
// Input file, little endian: u64 n, u64 nreads, u32 nref, u32 cases' expected `outside`; mg_aln_rec[n]; u64[2 * nreads]; u32[nref];
// u8[n] (1 = the definition keeps the record).  Every array is its own heap block of exactly that size, so that a read behind one
// is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_sidemask_core.h"

struct Word0 {
  const uint64_t* a;
  uint64_t operator[](uint64_t r) const { return a[2 * r]; }
};

template <class T> static bool read_block(FILE* f, T** out, uint64_t count) {
  *out = count ? static_cast<T*>(std::malloc(count * sizeof(T))) : nullptr;
  return count == 0 || std::fread(*out, sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0, nreads = 0;
  uint32_t nref = 0, want_outside = 0;
  if (std::fread(&n, 8, 1, f) != 1 || std::fread(&nreads, 8, 1, f) != 1 || std::fread(&nref, 4, 1, f) != 1 ||
      std::fread(&want_outside, 4, 1, f) != 1)
    return 2;
  mg_aln_rec* recs;
  uint64_t* words;
  uint32_t* ref2tax;
  uint8_t* want;
  if (!read_block(f, &recs, n) || !read_block(f, &words, 2 * nreads) || !read_block(f, &ref2tax, (uint64_t)nref) || !read_block(f, &want, n))
    return 2;
  std::fclose(f);

  // phase 1: NEW bits per tile
  const uint64_t ntiles = (n + mgs::kTile - 1) / mgs::kTile;
  std::vector<uint64_t> tile(ntiles, 0);
  for (uint64_t i = 0; i < n; ++i) tile[i / mgs::kTile] += mgs::is_new(recs[i]) ? 1u : 0u;
  // phase 2: their exclusive scan
  uint64_t run = 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    const uint64_t c = tile[t];
    tile[t] = run;
    run += c;
  }
  // phase 3: the prefix inside the tile, the decision, the masked copy
  const Word0 w0{words};
  uint64_t differ = 0, outside = 0, kept = 0;
  for (uint64_t t = 0; t < ntiles; ++t) {
    uint64_t seen = tile[t];
    const uint64_t end = (t + 1) * mgs::kTile < n ? (t + 1) * mgs::kTile : n;
    for (uint64_t i = t * mgs::kTile; i < end; ++i) {
      seen += mgs::is_new(recs[i]) ? 1u : 0u;
      const uint64_t ord = seen - 1;  // (2^64 - 1 in front of the first NEW record)
      const bool kp = mgs::keep(recs[i], ord, nreads, w0, ref2tax, nref);
      if (!mgs::in_range(ord, nreads)) ++outside;
      kept += kp;
      const mg_aln_rec out = kp ? recs[i] : mgs::masked(recs[i]);
      const bool same_but_the_bit = out.ref_new == recs[i].ref_new && out.matched == recs[i].matched && out.total == recs[i].total &&
                                    (out.flag_len & ~mgs::kMaskFlag) == (recs[i].flag_len & ~mgs::kMaskFlag) &&
                                    (kp ? out.flag_len == recs[i].flag_len : (out.flag_len & mgs::kMaskFlag) != 0);
      if (kp != (want[i] != 0) || !same_but_the_bit) {
        if (differ < 10) std::printf("record %llu: kept %d, the definition %d\n", (unsigned long long)i, (int)kp, (int)want[i]);
        ++differ;
      }
    }
  }
  if (outside != want_outside) {
    std::printf("outside %llu, the definition %u\n", (unsigned long long)outside, want_outside);
    ++differ;
  }
  std::free(recs);
  std::free(words);
  std::free(ref2tax);
  std::free(want);
  std::printf("%llu records, %llu kept, %llu differ\n", (unsigned long long)n, (unsigned long long)kept, (unsigned long long)differ);
  return differ ? 1 : 0;
}
