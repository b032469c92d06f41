// host_align_gap_check.cpp — mg_align_gap_core.h on the host (tests/test_align_gap_host.py builds this with the sanitizers and
// compares its output with metalign_amd/align.py: gap_cells and extend_gapped).  It fills the band as k_al_gap of mg_align.hip does:
// row by row, offset by offset, D from the prefix maximum of the row's offers, four remembered bits per cell, the best cell as the
// maximum of one packed number, the walk back from the bits alone.  Beside that it computes D by the definition's own rule
// (gap_del) and stops with exit code 4 where the two differ.  The case file, little endian:
//   u32 ncases, then per case: u32 P, B, O, E, i32 d, u32 L, u32 n, L codes of the oriented read, n codes of the accession
//     -> "G <case> <score> <b> <e> <nm> <pos0> <span> <ops>"  (ops: one of M I D per column, `*` for none)
//        "r <i> <cell> ..." for every row: 2B + 1 cells, `-` for one that does not exist, else H,I,D with `n` for no I / no D
// The read and the accession are heap blocks of exactly their size: a read outside them is the sanitizer's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../metalign_amd/csrc/mg_align_gap_core.h"

namespace {

std::vector<uint8_t> g_file;
size_t g_at = 0;

uint32_t u32() {
  uint32_t v;
  if (g_at + 4 > g_file.size()) {
    fprintf(stderr, "case file too short\n");
    exit(2);
  }
  memcpy(&v, g_file.data() + g_at, 4);
  g_at += 4;
  return v;
}

uint8_t* block(uint32_t n) {
  uint8_t* p = new uint8_t[n ? n : 1];
  if (g_at + n > g_file.size()) exit(2);
  memcpy(p, g_file.data() + g_at, n);
  g_at += n;
  return p;
}

void put(int32_t v) {
  if (v == mga::kGapNone) printf("n");
  else printf("%d", v);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  g_file.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (fread(g_file.data(), 1, g_file.size(), f) != g_file.size()) return 2;
  fclose(f);

  const uint32_t ncases = u32();
  for (uint32_t c = 0; c < ncases; ++c) {
    const int32_t P = (int32_t)u32(), B = (int32_t)u32(), O = (int32_t)u32(), E = (int32_t)u32(), d = (int32_t)u32();
    const int32_t L = (int32_t)u32(), n = (int32_t)u32();
    uint8_t* o = block((uint32_t)L);
    uint8_t* g = block((uint32_t)n);
    const int32_t T = 2 * B + 1;
    std::vector<int32_t> Hp(T, 0), Ip(T, mga::kGapNone), H(T), I(T), D(T);
    std::vector<uint8_t> bits((size_t)L * T, 0);
    std::vector<std::string> rows;
    uint32_t best = 0;
    for (int32_t i = 0; i < L; ++i) {
      std::vector<bool> ex(T);
      std::vector<int32_t> X(T), Hq(T);
      for (int32_t t = 0; t < T; ++t) {
        const int64_t j = (int64_t)i + d + t - B;
        ex[t] = j >= 0 && j < n;
        if (!ex[t]) continue;
        const bool up_ex = i > 0 && t < 2 * B;
        X[t] = Hp[t] + mga::gap_sub(o[i], g[j], P);
        I[t] = mga::gap_ins(up_ex, up_ex ? Hp[t + 1] : 0, up_ex ? Ip[t + 1] : 0, O, E);
        Hq[t] = mga::gap_max(mga::gap_max(0, X[t]), I[t]);
      }
      int32_t pm = mga::kGapNone;  // the largest offer of the offsets below t
      printf("r %d", i);
      for (int32_t t = 0; t < T; ++t) {
        if (!ex[t]) {
          H[t] = 0;
          I[t] = D[t] = mga::kGapNone;
          pm = mga::gap_max(pm, mga::gap_del_offer(false, 0, t, E));
          printf(" -");
          continue;
        }
        D[t] = mga::gap_del_prefix(pm, t, O, E);
        const bool left_ex = t > 0 && ex[t - 1];
        const int32_t serial = mga::gap_del(left_ex, left_ex ? H[t - 1] : 0, left_ex ? D[t - 1] : 0, O, E);
        if (serial != D[t]) {
          fprintf(stderr, "case %u cell (%d, %d): D %d from the prefix, %d by the definition's rule\n", c, i, t, D[t], serial);
          return 4;
        }
        H[t] = mga::gap_h(X[t], I[t], D[t]);
        bits[(size_t)i * T + t] = (uint8_t)mga::gap_bits(H[t], X[t], I[t], D[t], Hp[t], t < 2 * B ? Hp[t + 1] : 0, t > 0 ? H[t - 1] : 0, O, E);
        if (H[t] > 0) {
          const uint32_t key = mga::gap_best_pack(H[t], i, t);
          best = key > best ? key : best;
        }
        pm = mga::gap_max(pm, mga::gap_del_offer(true, Hq[t], t, E));
        printf(" ");
        put(H[t]);
        printf(",");
        put(I[t]);
        printf(",");
        put(D[t]);
      }
      printf("\n");
      for (int32_t t = 0; t < T; ++t) {
        Hp[t] = H[t];
        Ip[t] = ex[t] ? I[t] : mga::kGapNone;
      }
    }
    if (best == 0) {
      printf("G %u 0 0 0 0 0 0 *\n", c);
    } else {
      mga::GapWalk w;
      w.i = mga::gap_best_i(best);
      w.t = mga::gap_best_t(best);
      const int32_t e = w.i + 1;
      const int64_t j_end = (int64_t)w.i + d + w.t - B;
      std::string ops;
      uint32_t nm = 0;
      while (!w.done) {
        if (w.i < 0 || w.t < 0 || w.t >= T) {
          fprintf(stderr, "case %u: the walk left the band at (%d, %d)\n", c, w.i, w.t);
          return 5;
        }
        const int32_t ci = w.i, ct = w.t;
        const int32_t op = mga::gap_walk(w, bits[(size_t)ci * T + ct]);
        if (op < 0) continue;
        if (op == (int32_t)mga::kOpM) nm += mga::gap_sub(o[ci], g[(int64_t)ci + d + ct - B], P) < 0 ? 1u : 0u;
        else ++nm;
        ops.push_back("MID"[op]);
      }
      const int64_t pos0 = (int64_t)w.i + d + w.t - B;
      printf("G %u %d %d %d %u %lld %lld %s\n", c, mga::gap_best_h(best), w.i, e, nm, (long long)pos0, (long long)(j_end - pos0 + 1),
             std::string(ops.rbegin(), ops.rend()).c_str());
    }
    delete[] o;
    delete[] g;
  }
  printf("%u cases\n", ncases);
  return 0;
}
