// The read logic of the device's BAM reads path (metalign_amd/csrc/mg_bam_core.h: seq_kept / kept_len / seq_span / seq_base)
// compiled for the HOST: run by tests/test_bam_reads_host.py.
//
// Input file (little-endian): u32 n_ref, u64 n, n bytes of records (what follows a BAM header).  The chain is walked as the device
// walks it (mgb::walk over the whole range); every record is then read through an accessor that aborts on an offset outside the
// record's own bytes [p, p + 4 + block_size): no load of the read path may leave the record.  stdout: "chain <records> <end>
// <status>", then one line per kept read, "read <length> <bases>" (the bases in the read's own orientation, as k_bam_seq_unpack
// writes them; "-" for an empty read), and "kept <reads> <bases>" — what k_bam_seq_len and the two scans give.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../metalign_amd/csrc/mg_bam_core.h"

struct Guard {
  const uint8_t* p;
  uint64_t lo, hi;
  uint8_t operator[](uint64_t i) const {
    if (i < lo || i >= hi) {
      fprintf(stdout, "OOB load at %llu outside [%llu, %llu)\n", (unsigned long long)i, (unsigned long long)lo, (unsigned long long)hi);
      exit(3);
    }
    return p[i];
  }
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_ref = 0;
  uint64_t n = 0;
  if (fread(&n_ref, 4, 1, f) != 1 || fread(&n, 8, 1, f) != 1) return 2;
  std::vector<uint8_t> data(n + 1);
  if (n && fread(data.data(), 1, n, f) != n) return 2;
  fclose(f);
  const Guard all{data.data(), 0, n};
  std::vector<uint32_t> offs(n / mgb::kMinRecord + 2);
  uint64_t end = 0;
  int status = 0;
  const uint32_t nrec = mgb::walk(all, n, (int32_t)n_ref, 0, n, 0, offs.data(), (uint32_t)offs.size(), &end, &status);
  printf("chain %u %llu %d\n", nrec, (unsigned long long)end, status);
  uint64_t nreads = 0, nbases = 0;
  std::string out;
  for (uint32_t r = 0; r < nrec; ++r) {
    const uint64_t p = offs[r];
    const uint64_t bs = mgb::ld32(all, p);
    const Guard m{data.data(), p, p + 4 + bs};
    uint32_t kept = 0;
    const uint32_t len = mgb::kept_len(m, p, &kept);
    if (!kept) {
      if (len != 0) { printf("a record that is not a read has length %u\n", len); return 4; }
      continue;
    }
    uint64_t seq = 0;
    uint32_t lseq = 0, flag = 0;
    mgb::seq_span(m, p, &seq, &lseq, &flag);
    if (lseq != len || !mgb::seq_kept(flag)) { printf("kept_len and seq_span disagree\n"); return 4; }
    out.assign(len, '?');
    for (uint32_t j = 0; j < len; ++j) out[j] = (char)mgb::seq_base(m, seq, len, (flag & mgb::kFlagReverse) != 0, j);
    printf("read %u %s\n", len, len ? out.c_str() : "-");
    ++nreads;
    nbases += len;
  }
  printf("kept %llu %llu\n", (unsigned long long)nreads, (unsigned long long)nbases);
  return 0;
}
