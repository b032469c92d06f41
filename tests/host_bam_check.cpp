// The BAM record logic of the device (metalign_amd/csrc/mg_bam_core.h) compiled for the HOST: run by tests/test_bam_core_host.py.
//
// Input file (little-endian): u32 n_ref, i32 refmap[n_ref + 1], u64 n, n bytes of records, u32 nsizes, u32 chunk sizes[nsizes].
// For every chunk size it runs the device's scheme — a speculative entry per chunk (the first plausible start), the chain walked
// to the chunk's end, the chunks stitched in order and re-walked where the entry was wrong — and compares the record offsets, the
// end and the status with ONE sequential walk of the chain.  Every byte is read through an accessor that aborts on an offset
// outside [0, n): no check / walk / decode may load outside the range, whatever the bytes.  Then every record of the chain is
// decoded; stdout: "walk <size> ok" lines, "end <offset> <status>", and one "rec" line per record for the test to compare.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_bam_core.h"

struct Guard {
  const uint8_t* p;
  uint64_t n;
  uint8_t operator[](uint64_t i) const {
    if (i >= n) {
      fprintf(stdout, "OOB load at %llu of %llu\n", (unsigned long long)i, (unsigned long long)n);
      exit(3);
    }
    return p[i];
  }
};

struct Chain {
  std::vector<uint64_t> offs;
  uint64_t end = 0;
  int status = 0;
};

static Chain sequential(const Guard& m, uint64_t n, int32_t n_ref) {
  Chain c;
  std::vector<uint32_t> o(n / mgb::kMinRecord + 2);
  c.end = 0;
  const uint32_t k = mgb::walk(m, n, n_ref, 0, n, 0, o.data(), (uint32_t)o.size(), &c.end, &c.status);
  for (uint32_t i = 0; i < k; ++i) c.offs.push_back(o[i]);
  return c;
}

// k_bam_walk + k_bam_stitch, chunk by chunk
static Chain chunked(const Guard& m, uint64_t n, int32_t n_ref, uint32_t chunk) {
  const uint64_t nch = (n + chunk - 1) / chunk;
  const uint32_t cap = chunk / mgb::kMinRecord + 2;
  std::vector<uint64_t> entry(nch), exit(nch);
  std::vector<uint32_t> count(nch), offs(nch * cap);
  std::vector<int> status(nch);
  for (uint64_t j = 0; j < nch; ++j) {
    const uint64_t cs = j * chunk, ce = n - cs < chunk ? n : cs + chunk;
    uint64_t e = j == 0 ? 0 : mgb::find(m, n, n_ref, cs, ce);
    if (j && e == ce) e = ~0ull;
    uint64_t x = ce;
    int st = 0;
    count[j] = e == ~0ull ? 0 : mgb::walk(m, n, n_ref, e, ce, cs, offs.data() + j * cap, cap, &x, &st);
    entry[j] = e;
    exit[j] = x;
    status[j] = st;
  }
  Chain c;
  uint64_t want = 0;
  for (uint64_t j = 0; j < nch; ++j) {
    if (entry[j] != want) {  // re-walked from the true entry
      const uint64_t cs = j * chunk, ce = n - cs < chunk ? n : cs + chunk;
      uint64_t x = want;
      int st = 0;
      count[j] = mgb::walk(m, n, n_ref, want, ce, cs, offs.data() + j * cap, cap, &x, &st);
      exit[j] = x;
      status[j] = st;
    }
    for (uint32_t i = 0; i < count[j]; ++i) c.offs.push_back(j * chunk + offs[j * cap + i]);
    want = exit[j];
    c.status = status[j];
    if (status[j] == mgb::kBad) break;
  }
  c.end = want;
  return c;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_ref = 0;
  if (fread(&n_ref, 4, 1, f) != 1) return 2;
  std::vector<int32_t> refmap(n_ref + 1);
  uint64_t n = 0;
  if (fread(refmap.data(), 4, n_ref + 1, f) != n_ref + 1 || fread(&n, 8, 1, f) != 1) return 2;
  std::vector<uint8_t> bytes(n + 1);
  uint32_t nsizes = 0;
  if ((n && fread(bytes.data(), 1, n, f) != n) || fread(&nsizes, 4, 1, f) != 1) return 2;
  std::vector<uint32_t> sizes(nsizes);
  if (nsizes && fread(sizes.data(), 4, nsizes, f) != nsizes) return 2;
  fclose(f);
  const Guard m{bytes.data(), n};
  const Chain seq = sequential(m, n, (int32_t)n_ref);
  for (uint32_t s : sizes) {
    const Chain c = chunked(m, n, (int32_t)n_ref, s);
    const bool same = c.offs == seq.offs && c.end == seq.end && c.status == seq.status;
    printf("walk %u %s\n", s, same ? "ok" : "FAIL");
  }
  // a plausible start is a record inside the range: for every offset and a few cut ranges
  bool inside = true;
  for (uint64_t cut : {n, n - n / 3, n / 2, n / 7}) {
    const Guard g{bytes.data(), cut};
    for (uint64_t q = 0; q <= cut; ++q) {
      uint64_t nx = 0;
      if (mgb::check(g, cut, q, (int32_t)n_ref, &nx) == mgb::kOk && (nx > cut || nx < q + mgb::kMinRecord)) inside = false;
    }
  }
  printf("inside %s\n", inside ? "ok" : "FAIL");
  printf("end %llu %d\n", (unsigned long long)seq.end, seq.status);
  for (uint64_t p : seq.offs) {
    mgb::Decoded d;
    mgb::decode(m, n, p, refmap.data(), (int32_t)n_ref, &d);
    printf("rec %llu %u %u %u %u %u %u %llu %u\n", (unsigned long long)p, d.kind, d.retained, d.rec.ref_new, d.rec.matched,
           d.rec.total, d.rec.flag_len, (unsigned long long)d.qbeg, d.qlen);
  }
  return 0;
}
