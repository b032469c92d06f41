// host_align_pair_check.cpp — mg_align_pair_core.h on the host (tests/test_align_pair_host.py builds this with the sanitizers and
// compares its output with metalign_amd/align.py: rescue_window, concordant, select_pair and pair_flag).  It chooses a pair's
// records as k_al_select_pair of mg_align.hip does: the best concordant pair of the two lists, the secondaries by their best
// concordant partner, or each mate alone.  The case file is text, integers separated by white space:
//   W strand d L Lp n I                     -> "W <ok> <lo> <hi>"
//   C <alignment x> <alignment y> I         -> "C <0 / 1>"            an alignment: a strand score pos0 span b e L
//   P I sec_pct max_secondary n1 L1 n2 L2, then n1 + n2 entries: a strand score pos0 span b e
//                                           -> "P <proper> <best> | <entry:flag> ... | <entry:flag> ..."  (the kept entries of
//                                              each list in the order of their records, with their FLAG bits)
// Every list is a heap block of exactly its size: a read outside it is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metalign_amd/csrc/mg_align_pair_core.h"

namespace {

FILE* g_in;

long long num() {
  long long v;
  if (fscanf(g_in, "%lld", &v) != 1) {
    fprintf(stderr, "case file too short\n");
    exit(2);
  }
  return v;
}

mga::PairAln aln(uint32_t L) {
  const uint32_t a = (uint32_t)num(), strand = (uint32_t)num(), score = (uint32_t)num(), pos0 = (uint32_t)num(), span = (uint32_t)num();
  const uint32_t b = (uint32_t)num(), e = (uint32_t)num();
  return mga::pair_aln(a, strand, score, pos0, span, b, e, L);
}

struct ListAt {
  const mga::PairAln* p;
  mga::PairAln operator()(uint32_t i) const { return p[i]; }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  g_in = fopen(argv[1], "r");
  if (!g_in) return 2;
  char kind;
  unsigned ncases = 0;
  while (fscanf(g_in, " %c", &kind) == 1) {
    ++ncases;
    if (kind == 'W') {
      const uint32_t strand = (uint32_t)num();
      const int64_t d = num(), L = num(), Lp = num(), n = num(), I = num();
      int64_t lo = 0, hi = 0;
      const bool ok = mga::rescue_window(strand, d, L, Lp, n, I, &lo, &hi);
      printf("W %d %lld %lld\n", ok ? 1 : 0, (long long)lo, (long long)hi);
    } else if (kind == 'C') {
      mga::PairAln x, y;
      for (mga::PairAln* z : {&x, &y}) {
        long long f[7];
        for (long long& v : f) v = num();
        *z = mga::pair_aln((uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[3], (uint32_t)f[4], (uint32_t)f[5], (uint32_t)f[6],
                           (uint32_t)num());
      }
      printf("C %d\n", mga::concordant(x, y, num()) ? 1 : 0);
    } else if (kind == 'P') {
      const int64_t I = num();
      const uint32_t sec_pct = (uint32_t)num(), max_secondary = (uint32_t)num();
      uint32_t cnt[2], L[2];
      mga::PairAln* lists[2];
      cnt[0] = (uint32_t)num();
      L[0] = (uint32_t)num();
      cnt[1] = (uint32_t)num();
      L[1] = (uint32_t)num();
      for (int m = 0; m < 2; ++m) {
        lists[m] = new mga::PairAln[cnt[m] ? cnt[m] : 1];
        for (uint32_t i = 0; i < cnt[m]; ++i) lists[m][i] = aln(L[m]);
      }
      const ListAt at[2] = {{lists[0]}, {lists[1]}};
      uint32_t own[2] = {0, 0}, best = 0;
      const bool proper = mga::pair_best(at[0], cnt[0], at[1], cnt[1], I, &own[0], &own[1], &best);
      std::vector<uint32_t> kept[2];
      for (int m = 0; m < 2; ++m) {
        if (proper) {
          kept[m].push_back(own[m]);
          for (uint32_t t = 0; t < cnt[m] && kept[m].size() < 1 + max_secondary; ++t) {
            if (t == own[m]) continue;
            uint32_t partner = 0;
            if (mga::pair_partner(lists[m][t], at[1 - m], cnt[1 - m], I, &partner) &&
                mga::pair_secondary_ok(lists[m][t].score, partner, best, sec_pct))
              kept[m].push_back(t);
          }
        } else if (cnt[m]) {
          kept[m].push_back(0);
          for (uint32_t t = 1; t < cnt[m] && kept[m].size() < 1 + max_secondary; ++t)
            if (mga::secondary_ok(lists[m][t].score, lists[m][0].score, sec_pct)) kept[m].push_back(t);
        }
      }
      printf("P %d %u", proper ? 1 : 0, best);
      for (int m = 0; m < 2; ++m) {
        printf(" |");
        const bool partner_has = !kept[1 - m].empty();
        const uint32_t partner_strand = partner_has ? lists[1 - m][kept[1 - m][0]].strand : 0;
        for (size_t t = 0; t < kept[m].size(); ++t)
          printf(" %u:%u", kept[m][t],
                 mga::pair_flag((uint32_t)m, (uint32_t)t, lists[m][kept[m][t]].strand, partner_has, partner_strand, proper));
      }
      printf("\n");
      delete[] lists[0];
      delete[] lists[1];
    } else {
      fprintf(stderr, "unknown case kind %c\n", kind);
      return 2;
    }
  }
  fclose(g_in);
  printf("%u cases\n", ncases);
  return 0;
}
