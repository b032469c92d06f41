// The collation's per-record logic (metalign_amd/csrc/mg_collate_core.h) compiled for the HOST: the QNAME key of every name of the
// input, through an accessor that refuses any byte outside the name, and the class of every FLAG from 0 to 4095.
// Input: u32 count, then per name u32 length + bytes.  Output: "seed S", "key LO HI" per name, "classes" + 4096 digits.
// Driven by tests/test_collate_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_collate_core.h"

struct Checked {
  const unsigned char* p;
  uint64_t beg, end;
  unsigned char operator[](uint64_t i) const {
    if (i < beg || i >= end) { printf("load outside the name at %llu\n", (unsigned long long)i); exit(2); }
    return p[i];
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  std::vector<unsigned char> buf;
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  printf("seed %u\n", mgc::kSeed);
  uint32_t count = 0;
  memcpy(&count, buf.data(), 4);
  uint64_t at = 4;
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t len = 0;
    memcpy(&len, buf.data() + at, 4);
    at += 4;
    const Checked m{buf.data(), at, at + len};
    uint64_t lo = 0, hi = 0;
    mgc::qname_key(m, at, len, &lo, &hi);
    printf("key %llu %llu\n", (unsigned long long)lo, (unsigned long long)hi);
    at += len;
  }
  printf("classes ");
  for (uint32_t flag = 0; flag < 4096; ++flag) printf("%u", mgc::rec_class(flag));
  printf("\n");
  return 0;
}
