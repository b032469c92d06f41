// host_multimap_check.cpp — mg_multimap_core.h on the host (tests/test_multimap_iter_host.py compiles this twice, plain and with
// -fsanitize=address,undefined, and compares what it prints with metalign_amd/multimap.py).
//
// Input file (little endian):
//   u32 ntax, then per taxon f64 w0, f64 w_prev, f64 extra
//   u32 nshares, then per share f64 w, f64 den, f64 hitlen, f64 genome_len (0: none)
//   u32 nstops, then per question u32 i, u32 max_iter, f64 tol, f64 change
//   u32 nlists, then per list u32 n and n x u32 (ascending, distinct)
// Output: "W <hex float>" per taxon (w_i), "C <hex float>" (change_i), "P <hex float>" per share, "S 0|1" per question,
// "H <hash>" per list.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metalign_amd/csrc/mg_multimap_core.h"

namespace {

struct In {
  std::vector<unsigned char> b;
  size_t p = 0;
  template <class T> T get() {
    if (p + sizeof(T) > b.size()) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    T v;
    std::memcpy(&v, b.data() + p, sizeof(T));
    p += sizeof(T);
    return v;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  In in;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) in.b.insert(in.b.end(), buf, buf + n);
    std::fclose(f);
  }
  const uint32_t ntax = in.get<uint32_t>();
  double change = 0.0;
  for (uint32_t t = 0; t < ntax; ++t) {
    const double w0 = in.get<double>(), w_prev = in.get<double>(), extra = in.get<double>();
    const double wn = mgm::has_entry(w0) ? mgm::next_weight(w0, extra) : w0;
    const double d = mgm::rel_change(wn, w_prev);
    if (d > change) change = d;
    std::printf("W %a\n", wn);
  }
  std::printf("C %a\n", change);
  const uint32_t nshares = in.get<uint32_t>();
  for (uint32_t k = 0; k < nshares; ++k) {
    const double w = in.get<double>(), den = in.get<double>(), hitlen = in.get<double>(), gl = in.get<double>();
    std::printf("P %a\n", mgm::share(w, den, hitlen, gl != 0.0 ? &gl : nullptr, 0));
  }
  const uint32_t nstops = in.get<uint32_t>();
  for (uint32_t k = 0; k < nstops; ++k) {
    const uint32_t i = in.get<uint32_t>(), max_iter = in.get<uint32_t>();
    const double tol = in.get<double>(), c = in.get<double>();
    std::printf("S %d\n", mgm::stop_after(i, max_iter, tol, c) ? 1 : 0);
  }
  const uint32_t nlists = in.get<uint32_t>();
  for (uint32_t k = 0; k < nlists; ++k) {
    const uint32_t n = in.get<uint32_t>();
    std::vector<uint32_t> taxa(n);
    for (uint32_t j = 0; j < n; ++j) taxa[j] = in.get<uint32_t>();
    std::printf("H %llu\n", (unsigned long long)mgm::list_hash(taxa, (uint64_t)n));
  }
  return 0;
}
