// mg_multimap_core.h — the loop arithmetic of the iterated multimapped-read reassignment (--multimap_iterations;
// metalign_amd/multimap.py is the definition): what the host routine (mg_multimapped_shares_iter), the device kernels
// (k_mm_class_step, k_mm_update: mg_multimap.hip) and the stand-alone checker (tests/host_multimap_check.cpp) decide per taxon
// and per iteration.
//
//   has_entry()    a weight that is not NaN: the taxon has an entry in taxids2abs
//   share()        one taxon's part of one read (or of one class of reads): (w / den) * hitlen [/ genome length]
//   next_weight()  w_i = w0 + extra_i (an untouched taxon has extra_i = +0.0: w0 + 0.0 == w0 for the weights >= 0 there are)
//   rel_change()   |w_i - w_{i-1}| / w_i; 0 for a taxon without an entry or with w_i == 0
//   stop_after()   the stop rule: i == max_iter, or tol > 0 and change_i <= tol
//   list_hash()    64-bit hash of a sorted list of distinct taxa (the device's class key; never all-ones, which marks the empty list)
//
// Written so that the SAME code compiles for the host and for gfx950; no fused multiply-add may join a share to the sum it
// goes into (the including file sets `fp contract(off)` around its host loop; the functions here have one rounding per line).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MGM_HD __host__ __device__ inline
#else
#define MGM_HD inline
#endif

namespace mgm {

constexpr uint64_t kEmptyListHash = ~0ull;

MGM_HD bool has_entry(double w) { return w == w; }

MGM_HD double share(double w, double den, double hitlen, const double* genome_len, uint32_t t) {
  const double frac = w / den;
  double part = frac * hitlen;
  if (genome_len) part = part / genome_len[t];
  return part;
}

MGM_HD double next_weight(double w0, double extra) { return w0 + extra; }

MGM_HD double rel_change(double w_new, double w_old) {
  if (!has_entry(w_new) || w_new == 0.0) return 0.0;
  const double d = w_new - w_old;
  return (d < 0.0 ? -d : d) / w_new;
}

MGM_HD bool stop_after(uint32_t i, uint32_t max_iter, double tol, double change) {
  return i >= max_iter || (tol > 0.0 && change <= tol);
}

MGM_HD uint64_t hash_step(uint64_t h, uint32_t t) {
  h = (h ^ (uint64_t)t) * 0xff51afd7ed558ccdull;
  return h ^ (h >> 29);
}

// taxa[0..n): ascending, distinct, n >= 1
template <class L> MGM_HD uint64_t list_hash(const L& taxa, uint64_t n) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ n;
  for (uint64_t i = 0; i < n; ++i) h = hash_step(h, taxa[i]);
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 32;
  return h == kEmptyListHash ? 0ull : h;
}

}  // namespace mgm
