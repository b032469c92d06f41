// mg_multimap.hip — multimapped-read reassignment run to a fixed point (--multimap_iterations; metalign_amd/multimap.py is the
// definition, mg_multimap_core.h the arithmetic host and device share).
//
// Host: mg_multimapped_shares_iter loops mg_multimapped_shares (mg_profile.hip), bit for bit the definition.
//
// Device: an iteration runs over EQUIVALENCE CLASSES of reads, not over reads.  Which taxa have an entry never changes between
// iterations, so a read's sorted list of distinct kept taxa is fixed, and all reads with the same list get the same shares up to
// the factor hitlen: sum_r (w/den) * hitlen_r = (w/den) * sum_r hitlen_r, the last sum an exact integer.  Built once per call:
//   1. k_mm_rows / k_mm_first   one thread per ENTRY: is it the first occurrence in its read of a taxon that has a weight?  (a long
//                               list is spread over as many threads as it has entries; no per-thread array of any size)
//   2. scan of the per-read counts, k_mm_canon: every first occurrence goes to its rank among the read's distinct taxa — the
//      sorted distinct list, compacted; k_mm_hash: 64-bit hash of that list (all-ones: the empty list)
//   3. sort_pairs (hash, read); k_mm_heads marks a head where the hash OR THE LIST ITSELF differs from the previous read's: a hash
//      collision can only split a class (two equal lists that are not neighbours in the sorted order), never merge two lists
//   4. scan of the heads, k_mm_classes: representative read, list length and the u64 sum of hitlen per class (a segmented sum
//      inside each wavefront, one atomic per wavefront and class); k_mm_class_lists copies the lists class after class, so that
//      an iteration streams them
// Per iteration: k_mm_class_step (one thread per class: den, the shares, f64 accumulation in LDS for ntax <= 2048, else global
// atomics — as k_resolve_multimapped) and k_mm_update (w_i = w0 + extra_i, the maximum relative change, zeroes the
// other accumulator).  The host reads one double back per iteration when tol > 0, one at the end when tol == 0.
#include <hip/hip_runtime.h>

#include <vector>

#include "mg_internal.h"
#include "mg_multimap_core.h"

namespace mg {
namespace {

constexpr unsigned kMB = 256;

__global__ __launch_bounds__(kMB) void k_mm_rows(const uint64_t* __restrict__ off, uint64_t nreads, uint32_t* __restrict__ rid,
                                                 uint32_t* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nreads; i += stride) {
    for (uint64_t e = off[i]; e < off[i + 1]; ++e) rid[e] = (uint32_t)i;
    cnt[i] = 0;
  }
}

// first[e] = 1: entry e names a taxon that has a weight, and no earlier entry of the read names it
__global__ __launch_bounds__(kMB) void k_mm_first(const uint64_t* __restrict__ off, const uint32_t* __restrict__ tax,
                                                  const uint32_t* __restrict__ rid, uint64_t nent,
                                                  const double* __restrict__ weight, uint32_t ntax, uint8_t* __restrict__ first,
                                                  uint32_t* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nent; e += stride) {
    const uint32_t r = rid[e], t = tax[e];
    bool keep = t < ntax && mgm::has_entry(weight[t]);
    if (keep)
      for (uint64_t f = off[r]; f < e; ++f)
        if (tax[f] == t) { keep = false; break; }
    first[e] = keep ? 1 : 0;
    if (keep) atomicAdd(&cnt[r], 1u);
  }
}

// lists[coff[r] + rank] = t: rank = the distinct kept taxa of the read below t (rank < cnt[r] = coff[r + 1] - coff[r])
__global__ __launch_bounds__(kMB) void k_mm_canon(const uint64_t* __restrict__ off, const uint32_t* __restrict__ tax,
                                                  const uint32_t* __restrict__ rid, const uint8_t* __restrict__ first,
                                                  uint64_t nent, const uint64_t* __restrict__ coff, uint32_t* __restrict__ lists) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nent; e += stride) {
    if (!first[e]) continue;
    const uint32_t r = rid[e], t = tax[e];
    const uint64_t o0 = off[r], o1 = off[r + 1];
    uint64_t rank = 0;
    for (uint64_t g = o0; g < o1; ++g) rank += (first[g] && tax[g] < t) ? 1u : 0u;
    lists[coff[r] + rank] = t;
  }
}

__global__ __launch_bounds__(kMB) void k_mm_hash(const uint64_t* __restrict__ coff, const uint32_t* __restrict__ lists,
                                                 uint64_t nreads, uint64_t mask, uint64_t* __restrict__ keys,
                                                 uint32_t* __restrict__ vals) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nreads; i += stride) {
    const uint64_t c0 = coff[i], n = coff[i + 1] - c0;
    uint64_t h = mgm::kEmptyListHash;
    if (n) {
      h = mgm::list_hash(lists + c0, n) & mask;
      if (h == mgm::kEmptyListHash) h = 0;
    }
    keys[i] = h;
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(kMB) void k_mm_heads(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  uint64_t nreads, const uint64_t* __restrict__ coff,
                                                  const uint32_t* __restrict__ lists, uint32_t* __restrict__ head) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nreads; i += stride) {
    uint32_t h = 1;
    if (i > 0 && keys[i] == keys[i - 1]) {
      const uint32_t r = vals[i], q = vals[i - 1];
      const uint64_t a = coff[r], b = coff[q], n = coff[r + 1] - a;
      if (n == coff[q + 1] - b) {
        h = 0;
        for (uint64_t k = 0; k < n; ++k)
          if (lists[a + k] != lists[b + k]) { h = 1; break; }
      }
    }
    head[i] = h;
  }
}

// class of sorted read i = hscan[i] + head[i] - 1 (hscan: exclusive sums of head).  The hitlen sum: the classes are runs of the
// sorted order, so inside a wavefront a segmented inclusive scan leaves every run's sum in its last lane.
__global__ __launch_bounds__(kMB) void k_mm_classes(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ head,
                                                    const uint64_t* __restrict__ hscan, uint64_t nreads,
                                                    const uint64_t* __restrict__ coff, const uint64_t* __restrict__ hitlen,
                                                    uint32_t* __restrict__ crep, uint32_t* __restrict__ clen,
                                                    unsigned long long* __restrict__ chit) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t rounded = (nreads + 63) / 64 * 64;  // whole wavefronts take every trip of the loop together
  const unsigned lane = threadIdx.x & 63u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rounded; i += stride) {
    const bool valid = i < nreads;
    unsigned long long cid = ~0ull, sum = 0;
    if (valid) {
      const uint32_t r = vals[i];
      cid = hscan[i] + head[i] - 1;
      sum = hitlen[r];
      if (head[i]) { crep[cid] = r; clen[cid] = (uint32_t)(coff[r + 1] - coff[r]); }
    }
    for (unsigned d = 1; d < 64; d <<= 1) {
      const unsigned long long us = __shfl_up(sum, d, 64), uc = __shfl_up(cid, d, 64);
      if (lane >= d && uc == cid) sum += us;
    }
    const unsigned long long nc = __shfl_down(cid, 1, 64);
    if (valid && (lane == 63 || nc != cid)) atomicAdd(&chit[cid], sum);
  }
}

__global__ __launch_bounds__(kMB) void k_mm_class_lists(const uint32_t* __restrict__ crep, const uint64_t* __restrict__ cls_off,
                                                        uint64_t ncls, const uint64_t* __restrict__ coff,
                                                        const uint32_t* __restrict__ lists, uint32_t* __restrict__ clists) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncls; c += stride) {
    const uint64_t a = coff[crep[c]], b = cls_off[c], n = cls_off[c + 1] - b;
    for (uint64_t k = 0; k < n; ++k) clists[b + k] = lists[a + k];
  }
}

// One iteration's additions: one thread per class.  A class whose weights sum to 0 (or the class of the empty list) is skipped —
// decided anew with every iteration's weights.
__global__ __launch_bounds__(kMB) void k_mm_class_step(const uint64_t* __restrict__ cls_off, const uint32_t* __restrict__ clists,
                                                       const unsigned long long* __restrict__ chit, uint64_t ncls,
                                                       const double* __restrict__ weight, const double* __restrict__ genome_len,
                                                       uint32_t ntax, uint32_t use_lds, double* __restrict__ extra) {
  extern __shared__ double s_extra[];
  if (use_lds) {
    for (uint32_t t = threadIdx.x; t < ntax; t += blockDim.x) s_extra[t] = 0.0;
    __syncthreads();
  }
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncls; c += stride) {
    const uint64_t o0 = cls_off[c], o1 = cls_off[c + 1];
    double den = 0.0;
    for (uint64_t e = o0; e < o1; ++e) den += weight[clists[e]];
    if (den == 0.0) continue;
    const double hitlen = (double)chit[c];
    for (uint64_t e = o0; e < o1; ++e) {
      const uint32_t t = clists[e];
      const double part = mgm::share(weight[t], den, hitlen, genome_len, t);
      if (use_lds) atomicAdd(&s_extra[t], part); else atomicAdd(&extra[t], part);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < ntax; t += blockDim.x)
      if (s_extra[t] != 0.0) atomicAdd(&extra[t], s_extra[t]);
  }
}

// w_i = w0 + extra_i, change_i, and the other accumulator zeroed for iteration i + 1.  The maximum: per wavefront by shuffles, then one
// atomic per wavefront on the bits of the double (a change is never negative, so its bits order as it does); `change` was zeroed
// by the update before (or by the host, for the first), and this one zeroes the slot of the next.
__global__ __launch_bounds__(kMB) void k_mm_update(const double* __restrict__ w0, const double* __restrict__ w_prev,
                                                   double* __restrict__ w_next, const double* __restrict__ extra,
                                                   double* __restrict__ extra_next, uint32_t ntax,
                                                   unsigned long long* __restrict__ change,
                                                   unsigned long long* __restrict__ change_next) {
  double c = 0.0;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < ntax; t += stride) {
    const double a = w0[t];
    const double wn = mgm::has_entry(a) ? mgm::next_weight(a, extra[t]) : a;
    w_next[t] = wn;
    const double d = mgm::rel_change(wn, w_prev[t]);
    if (d > c) c = d;
    extra_next[t] = 0.0;
  }
  for (unsigned d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_down(c, d, 64);
    if (o > c) c = o;
  }
  if ((threadIdx.x & 63u) == 0 && c > 0.0) atomicMax(change, (unsigned long long)__double_as_longlong(c));
  if (blockIdx.x == 0 && threadIdx.x == 0) *change_next = 0ull;
}

#define MM_LAUNCH(kernel, items, stream, ...)                                                                        \
  do {                                                                                                               \
    hipLaunchKernelGGL(kernel, dim3(grid_for((items), kMB, (unsigned)ctx().num_cus * 8)), dim3(kMB), 0, (stream), __VA_ARGS__); \
    MG_HIP(hipGetLastError());                                                                                       \
  } while (0)

}  // namespace

// The device loop over the multimapped CSR of a committed shard (mg_profile_mm_iterate_dev unpacks the handle: mg_profile.hip).
int mm_iterate_dev(const uint64_t* mm_offsets, const uint32_t* mm_tax, const uint64_t* mm_hitlen, uint64_t nreads, uint64_t nent,
                   uint32_t ntax, const double* d_weight0, const double* d_genome_len, uint32_t max_iter, double tol,
                   double* d_extra, uint32_t* iterations_run, double* last_change, uint64_t* nclasses) {
  hipStream_t st = stage_c_stream();
  MG_HIP(hipMemsetAsync(d_extra, 0, (uint64_t)ntax * sizeof(double), st));
  if (nclasses) *nclasses = 0;
  if (nreads == 0 || ntax == 0) {  // nothing is ever added: every w_i = w0, every change 0
    *iterations_run = tol > 0.0 ? 1u : max_iter;
    *last_change = 0.0;
    MG_HIP(hipStreamSynchronize(st));  // (the contract: the call returns with its work done — d_extra is zero)
    return MG_OK;
  }
  if (nreads >= 0xffffffffull) return fail(MG_ERR_CAPACITY, "%llu multimapped reads exceed 2^32-2", (unsigned long long)nreads);
  // ---- the classes (the sort and scan services run on the library stream: it waits for stage C's, and is waited for below)
  hipStream_t sb = ctx().stream;
  MG_TRY(mg_stage_c_join());
  DevBuf b_rid, b_first, b_cnt, b_coff, b_lists, b_keys, b_keys_s, b_vals, b_vals_s, b_head, b_hscan;
  MG_TRY(b_rid.alloc((nent + 1) * sizeof(uint32_t)));
  MG_TRY(b_first.alloc(nent + 1));
  MG_TRY(b_cnt.alloc(nreads * sizeof(uint32_t)));
  MG_TRY(b_coff.alloc((nreads + 1) * sizeof(uint64_t)));
  uint32_t* rid = b_rid.as<uint32_t>();
  uint8_t* first = b_first.as<uint8_t>();
  uint32_t* cnt = b_cnt.as<uint32_t>();
  uint64_t* coff = b_coff.as<uint64_t>();
  uint64_t nkept = 0;
  {
    ProfScope ps("mm_classes", sb);
    MM_LAUNCH(k_mm_rows, nreads, sb, mm_offsets, nreads, rid, cnt);
    if (nent) MM_LAUNCH(k_mm_first, nent, sb, mm_offsets, mm_tax, rid, nent, d_weight0, ntax, first, cnt);
    MG_TRY(exclusive_sum_u32_to_u64(cnt, coff, nreads, &nkept));
    if (nkept > nent) return fail(MG_ERR_STATE, "multimapped lists grew while they were made canonical");
    MG_TRY(b_lists.alloc((nkept + 1) * sizeof(uint32_t)));
    MG_TRY(b_keys.alloc(nreads * sizeof(uint64_t)));
    MG_TRY(b_keys_s.alloc(nreads * sizeof(uint64_t)));
    MG_TRY(b_vals.alloc(nreads * sizeof(uint32_t)));
    MG_TRY(b_vals_s.alloc(nreads * sizeof(uint32_t)));
    MG_TRY(b_head.alloc(nreads * sizeof(uint32_t)));
    MG_TRY(b_hscan.alloc((nreads + 1) * sizeof(uint64_t)));
  }
  uint32_t* lists = b_lists.as<uint32_t>();
  uint64_t ncls = 0, nclass_ent = 0;
  DevBuf b_crep, b_clen, b_chit, b_cls_off, b_clists;
  {
    ProfScope ps("mm_classes", sb);
    if (nent) MM_LAUNCH(k_mm_canon, nent, sb, mm_offsets, mm_tax, rid, first, nent, coff, lists);
    const int64_t bits = dbg("mm_hash_bits");  // (tests: a hash of few bits, so that different lists collide)
    const uint64_t mask = bits > 0 && bits < 64 ? (1ull << bits) - 1 : ~0ull;
    MM_LAUNCH(k_mm_hash, nreads, sb, coff, lists, nreads, mask, b_keys.as<uint64_t>(), b_vals.as<uint32_t>());
    MG_TRY(sort_pairs(b_keys.as<uint64_t>(), b_keys_s.as<uint64_t>(), b_vals.as<uint32_t>(), b_vals_s.as<uint32_t>(), nreads));
    MM_LAUNCH(k_mm_heads, nreads, sb, b_keys_s.as<uint64_t>(), b_vals_s.as<uint32_t>(), nreads, coff, lists, b_head.as<uint32_t>());
    MG_TRY(exclusive_sum_u32_to_u64(b_head.as<uint32_t>(), b_hscan.as<uint64_t>(), nreads, &ncls));
    if (ncls == 0 || ncls > nreads) return fail(MG_ERR_STATE, "%llu classes of %llu reads", (unsigned long long)ncls, (unsigned long long)nreads);
    MG_TRY(b_crep.alloc(ncls * sizeof(uint32_t)));
    MG_TRY(b_clen.alloc(ncls * sizeof(uint32_t)));
    MG_TRY(b_chit.alloc(ncls * sizeof(unsigned long long)));
    MG_TRY(b_cls_off.alloc((ncls + 1) * sizeof(uint64_t)));
    MG_HIP(hipMemsetAsync(b_chit.p, 0, ncls * sizeof(unsigned long long), sb));
    MM_LAUNCH(k_mm_classes, nreads, sb, b_vals_s.as<uint32_t>(), b_head.as<uint32_t>(), b_hscan.as<uint64_t>(), nreads, coff,
              mm_hitlen, b_crep.as<uint32_t>(), b_clen.as<uint32_t>(), b_chit.as<unsigned long long>());
    MG_TRY(exclusive_sum_u32_to_u64(b_clen.as<uint32_t>(), b_cls_off.as<uint64_t>(), ncls, &nclass_ent));
    if (nclass_ent > nkept) return fail(MG_ERR_STATE, "class lists longer than the reads' lists");
    MG_TRY(b_clists.alloc((nclass_ent + 1) * sizeof(uint32_t)));
    MM_LAUNCH(k_mm_class_lists, ncls, sb, b_crep.as<uint32_t>(), b_cls_off.as<uint64_t>(), ncls, coff, lists, b_clists.as<uint32_t>());
    // the empty list hashes to all-ones, above every other hash: its class, if there is one, is the last — and is not counted
    uint32_t* pin = reinterpret_cast<uint32_t*>(host_words() + kHostWordMmLastLen);
    MG_HIP(hipMemcpyAsync(pin, b_clen.as<uint32_t>() + (ncls - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, sb));
    MG_HIP(hipStreamSynchronize(sb));  // (and stage C's stream may go on from here)
    if (nclasses) *nclasses = ncls - (*pin == 0 ? 1 : 0);
  }
  // ---- the iterations
  DevBuf b_w, b_x, b_change;
  MG_TRY(b_w.alloc(2 * (uint64_t)ntax * sizeof(double)));
  MG_TRY(b_x.alloc(2 * (uint64_t)ntax * sizeof(double)));
  MG_TRY(b_change.alloc(2 * sizeof(double)));
  MG_HIP(hipMemsetAsync(b_change.p, 0, 2 * sizeof(double), st));
  double* wbuf[2] = {b_w.as<double>(), b_w.as<double>() + ntax};
  double* xbuf[2] = {b_x.as<double>(), b_x.as<double>() + ntax};
  MG_HIP(hipMemsetAsync(b_x.p, 0, 2 * (uint64_t)ntax * sizeof(double), st));
  const uint32_t use_lds = ntax <= 2048 ? 1u : 0u;
  const unsigned step_grid = grid_for(ncls, kMB, (unsigned)ctx().num_cus * 4);
  const unsigned update_grid = grid_for(ntax, kMB, (unsigned)ctx().num_cus * 4);
  double* pin_change = reinterpret_cast<double*>(host_words() + kHostWordMmChange);
  const double* cur = d_weight0;
  ProfScope ps("mm_iterate", st);
  for (uint32_t i = 1;; ++i) {
    double* x = xbuf[i & 1];
    hipLaunchKernelGGL(k_mm_class_step, dim3(step_grid), dim3(kMB), use_lds ? (size_t)ntax * sizeof(double) : 0, st,
                       b_cls_off.as<uint64_t>(), b_clists.as<uint32_t>(), b_chit.as<unsigned long long>(), ncls, cur, d_genome_len,
                       ntax, use_lds, x);
    MG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mm_update, dim3(update_grid), dim3(kMB), 0, st, d_weight0, cur, wbuf[i & 1], x, xbuf[(i + 1) & 1], ntax,
                       b_change.as<unsigned long long>() + (i & 1), b_change.as<unsigned long long>() + ((i + 1) & 1));
    MG_HIP(hipGetLastError());
    cur = wbuf[i & 1];
    const bool last = i >= max_iter;
    double change = 0.0;
    if (last || tol > 0.0) {  // (tol == 0: nothing is read back before the end)
      MG_HIP(hipMemcpyAsync(pin_change, b_change.as<double>() + (i & 1), sizeof(double), hipMemcpyDeviceToHost, st));
      MG_HIP(hipStreamSynchronize(st));
      change = *pin_change;
    }
    if (last || mgm::stop_after(i, max_iter, tol, change)) {
      MG_HIP(hipMemcpyAsync(d_extra, x, (uint64_t)ntax * sizeof(double), hipMemcpyDeviceToDevice, st));
      MG_HIP(hipStreamSynchronize(st));  // (the buffers go back to the pool)
      *iterations_run = i;
      *last_change = change;
      return MG_OK;
    }
  }
}

}  // namespace mg

using namespace mg;

extern "C" {

// (host code: every rounding is the definition's — no fused multiply-add anywhere in the loop)
#pragma clang fp contract(off)
int mg_multimapped_shares_iter(const uint64_t* mm_offsets, uint64_t nreads, const uint32_t* mm_tax, const uint64_t* mm_hitlen,
                               const double* weight, uint32_t ntax, const double* genome_len, uint32_t max_iter, double tol,
                               double* extra, uint8_t* touched, uint32_t* iterations_run, double* last_change) {
  if (!weight || !iterations_run || !last_change) return fail(MG_ERR_ARG, "null argument");
  if (max_iter < 1) return fail(MG_ERR_ARG, "max_iter must be at least 1");
  if (!(tol >= 0.0)) return fail(MG_ERR_ARG, "tol must not be negative");
  std::vector<double> w(weight, weight + ntax), wn(ntax);
  for (uint32_t i = 1;; ++i) {
    MG_TRY(mg_multimapped_shares(mm_offsets, nreads, mm_tax, mm_hitlen, w.data(), ntax, genome_len, extra, touched));
    double change = 0.0;
    for (uint32_t t = 0; t < ntax; ++t) {
      wn[t] = mgm::has_entry(weight[t]) ? mgm::next_weight(weight[t], extra[t]) : weight[t];
      const double d = mgm::rel_change(wn[t], w[t]);
      if (d > change) change = d;
    }
    w.swap(wn);
    if (mgm::stop_after(i, max_iter, tol, change)) {
      *iterations_run = i;
      *last_change = change;
      return MG_OK;
    }
  }
}

}  // extern "C"
