// The device algorithm of --depth (metalign_amd/csrc/mg_depth.hip) run serially on the HOST with the functions of
// mg_depth_core.h / mg_coverage_core.h: difference array over the slots, ONE flat inclusive scan, the extra slot of every accession
// skipped, the tiles without a hit accession left unread, histogram and windows.  Every slot access is checked against the array.
// Input: u32 W, u32 nacc, u64 lengths[nacc], u32 n, then per interval u32 row, u32 pos0, u32 span.
// Output: "U unplaced", then per accession with an alignment "A row alignments", "H row bin positions" per non-empty bin and
// "W row index depth_sum covered" per window with depth_sum > 0.
// Driven by tests/test_depth_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_depth_core.h"

static std::vector<unsigned char> buf;
static uint64_t at = 0;
template <class T> static T take() {
  T v;
  if (at + sizeof(T) > buf.size()) { printf("short input\n"); exit(3); }
  memcpy(&v, buf.data() + at, sizeof(T));
  at += sizeof(T);
  return v;
}

struct Slots {
  std::vector<int32_t> v;
  int32_t& operator[](uint64_t i) {
    if (i >= v.size()) { printf("slot %llu outside the array\n", (unsigned long long)i); exit(2); }
    return v[i];
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  const uint32_t W = take<uint32_t>(), nacc = take<uint32_t>();
  std::vector<uint64_t> len(nacc), off(nacc + 1, 0), woff(nacc + 1, 0), aln(nacc, 0);
  for (uint32_t a = 0; a < nacc; ++a) {
    len[a] = take<uint64_t>();
    off[a + 1] = off[a] + mgd::slots_of(len[a]);
    woff[a + 1] = woff[a] + mgd::windows_of_length(len[a], W);
  }
  Slots slots;
  slots.v.assign(off[nacc], 0);
  uint64_t unplaced = 0;
  for (uint32_t n = take<uint32_t>(), i = 0; i < n; ++i) {
    const uint32_t a = take<uint32_t>(), pos0 = take<uint32_t>(), span = take<uint32_t>();
    const uint64_t clen = a < nacc ? mgv::clipped(pos0, span, len[a]) : 0;
    if (!clen) { ++unplaced; continue; }
    uint64_t plus, minus;
    mgd::diff_slots(off[a], pos0, clen, &plus, &minus);
    if (plus < off[a] || minus >= off[a + 1]) { printf("interval outside its accession's slots\n"); return 2; }
    slots[plus] += 1;
    slots[minus] -= 1;
    ++aln[a];
  }
  // one flat scan, tile by tile as the device carries it
  std::vector<uint64_t> hist((uint64_t)nacc * mgd::kDepthBins, 0), wsum(woff[nacc], 0), wcov(woff[nacc], 0);
  std::vector<int32_t> rowmap(nacc, -1);
  for (uint32_t a = 0, r = 0; a < nacc; ++a)
    if (aln[a]) rowmap[a] = (int32_t)r++;
  long long carry = 0;
  for (uint64_t t = 0; t < mgd::tiles_of(off[nacc]); ++t) {
    uint64_t s = t * mgd::kTile;
    const uint64_t s_end = s + mgd::kTile < off[nacc] ? s + mgd::kTile : off[nacc];
    uint32_t a = mgv::owner_of(off, nacc, s);
    if (!(off[a] <= s && s < off[a + 1])) { printf("owner_of is wrong at slot %llu\n", (unsigned long long)s); return 2; }
    if (!mgd::tile_has_row(off, rowmap, nacc, a, s_end)) {  // (the device reads no slot of such a tile)
      for (; s < s_end; ++s)
        if (slots[s] != 0 || carry != 0) { printf("a tile without a row is not all zero\n"); return 2; }
      continue;
    }
    for (; s < s_end; ++s) {
      a = mgv::owner_from(off, nacc, a, s);
      carry += slots[s];
      if (carry < 0) { printf("negative depth\n"); return 2; }
      if (!mgd::is_base(s, off[a], len[a])) {
        if (carry != 0) { printf("an accession's slots do not sum to zero\n"); return 2; }
        continue;
      }
      ++hist[(uint64_t)a * mgd::kDepthBins + mgd::clamp((uint32_t)carry)];
      if (W && carry) {
        const uint64_t j = mgd::window_of(s - off[a], W);
        if (j >= woff[a + 1] - woff[a]) { printf("window outside its accession\n"); return 2; }
        wsum[woff[a] + j] += (uint64_t)carry;
        ++wcov[woff[a] + j];
      }
    }
  }
  printf("U %llu\n", (unsigned long long)unplaced);
  for (uint32_t a = 0; a < nacc; ++a) {
    if (!aln[a]) continue;
    printf("A %u %llu\n", a, (unsigned long long)aln[a]);
    for (uint32_t b = 0; b < mgd::kDepthBins; ++b)
      if (hist[(uint64_t)a * mgd::kDepthBins + b]) printf("H %u %u %llu\n", a, b, (unsigned long long)hist[(uint64_t)a * mgd::kDepthBins + b]);
    for (uint64_t g = woff[a]; g < woff[a + 1]; ++g)
      if (wsum[g]) printf("W %u %llu %llu %llu\n", a, (unsigned long long)(g - woff[a]), (unsigned long long)wsum[g], (unsigned long long)wcov[g]);
  }
  return 0;
}
