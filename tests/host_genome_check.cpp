// The per-line rules of the organism-file parser (metalign_amd/csrc/mg_genome_core.h) compiled for the HOST and run over the
// files of a case: tests/test_genome_core_host.py compares what this prints with build_db.genome_bases.
//
//   host_genome_check <cases.bin>     cases.bin: u32 nfiles, then per file u32 length + its bytes
//   prints per file   "undecided"  or  "bases <hex>"
//
// Every byte is read through a checked array: an index outside the file's buffer aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../metalign_amd/csrc/mg_genome_core.h"

struct Checked {
  const std::vector<uint8_t>* v;
  uint8_t operator[](uint64_t i) const {
    if (i >= v->size()) { fprintf(stderr, "index %llu outside a buffer of %zu bytes\n", (unsigned long long)i, v->size()); abort(); }
    return (*v)[i];
  }
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: host_genome_check <cases.bin>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t nfiles = 0;
  if (!rd(f, &nfiles, 4)) return 2;
  // the files back to back in ONE buffer, as the device has them: a file's last line must not run into the next file
  std::vector<uint8_t> all;
  std::vector<uint64_t> ext(1, 0);
  for (uint32_t i = 0; i < nfiles; ++i) {
    uint32_t len = 0;
    if (!rd(f, &len, 4)) return 2;
    all.resize(all.size() + len);
    if (!rd(f, all.data() + ext.back(), len)) return 2;
    ext.push_back(all.size());
  }
  fclose(f);
  const Checked m{&all};
  for (uint32_t i = 0; i < nfiles; ++i) {
    std::string out;
    const bool ok = mgg::genome_file(m, ext[i], ext[i + 1], [&](uint8_t b) {
      char h[3];
      snprintf(h, sizeof(h), "%02x", b);
      out += h;
    });
    if (ok) printf("bases %s\n", out.c_str());
    else printf("undecided\n");
  }
  return 0;
}
