// mg_side_dev.h — the device building blocks stage C's side outputs share (mg_coverage.hip, mg_depth.hip, mg_identity.hip,
// mg_variants.hip, mg_sidemask.hip): ONE copy of each, device-only.
//
//   wave_sum()          the sum of a 64-bit value over the wavefront's 64 lanes, in every lane
//   lds_probe()         the slot of a key in a hashed LDS key array: claimed with a CAS within kProbe slots of its hash, or none
//   AccBins             per-accession sums in hashed LDS bins.  Most records of a sample hit a few accessions, so plain global
//                       adds would pile onto a few cache lines: a wavefront whose records share one accession adds once, the others
//                       one by one into LDS, and every occupied bin gives one global add when the workgroup ends.  A key that
//                       finds no slot adds to memory directly, so the sums are EXACT whatever the contention and however many
//                       accessions there are — only the speed depends on the table's load.
//   WaveList            the wavefront's flattened work list: lane l brings len items, the lanes then stride the total, so
//                       neighbouring lanes take neighbouring items of one long record and no lane walks it alone
//   block_scan_excl()   the exclusive scan of an array in place by ONE workgroup walking it in steps: nobody waits for another
//                       workgroup, any length
//
// The search for the accession that owns an offset (mgv::owner_of, mgv::owner_from) is host and device code and lives in
// mg_coverage_core.h, where tests/host_depth_check.cpp checks it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mg {

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

constexpr unsigned kProbe = 8;

// The slot among keys[kSlots] (a power of two) that holds `key` or was empty and now does, looked for in the kProbe slots from
// h on; -1 when they all hold other keys.  kUnroll = 1 keeps it a loop — for the per-accession bins the first slot takes nearly every
// key and seven more copies of the CAS only lengthen the kernels; kUnroll = kProbe lays the probes out one behind the other, for a
// table loaded enough that later probes are usual (identity's (accession, bin) table).
template <unsigned kSlots, unsigned kUnroll = 1, class K> __device__ __forceinline__ int lds_probe(K* keys, K empty, K key, uint32_t h) {
  int slot = -1;
#pragma unroll kUnroll
  for (unsigned p = 0; p < kProbe && slot < 0; ++p) {
    const uint32_t s = (h + p) & (kSlots - 1);
    const K k = atomicCAS(&keys[s], empty, key);
    if (k == empty || k == key) slot = (int)s;
  }
  return slot;
}

// kVals 64-bit sums per accession — sum 0 is the number of records, the others are the caller's — and one counter of the records
// that belong to no accession (the unplaced, unscored, unpiled), for a workgroup of kThreads threads.  A __shared__ object:
//   bins.init();  loop { bins.count_one(miss); bins.add(active, a, more, global); }  bins.flush(global, miss_counter);
// count_one() and add() take the whole wavefront (they ballot); init() and flush() the whole workgroup (they hold its barriers).
template <unsigned kSlots, unsigned kVals, unsigned kThreads> struct AccBins {
  static_assert(kSlots >= 2 && (kSlots & (kSlots - 1)) == 0 && kVals >= 1, "a power of two of slots");
  static constexpr uint32_t kEmpty = 0xffffffffu;
  static constexpr unsigned kShift = 32 - __builtin_ctz(kSlots);
  uint32_t key[kSlots];
  unsigned long long val[kVals][kSlots];
  unsigned long long miss;

  __device__ __forceinline__ void init() {
    for (unsigned i = threadIdx.x; i < kSlots; i += kThreads) {
      key[i] = kEmpty;
      for (unsigned v = 0; v < kVals; ++v) val[v][i] = 0;
    }
    if (threadIdx.x == 0) miss = 0;
    __syncthreads();
  }

  // One LDS add per wavefront for its lanes with `flag`.
  __device__ __forceinline__ void count_one(bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63u) == (unsigned)__builtin_ctzll(m)) atomicAdd(&miss, (unsigned long long)__builtin_popcountll(m));
  }

  // Every active lane's record counts once for accession a and brings more[0 .. kVals - 1) for the sums behind the count.
  __device__ __forceinline__ void add(bool active, uint32_t a, const unsigned long long* more, unsigned long long* const* global) {
    const unsigned long long am = __ballot(active);
    if (!am) return;
    const unsigned lane = threadIdx.x & 63u, first = (unsigned)__builtin_ctzll(am);
    const uint32_t a_first = __shfl(a, (int)first, 64);
    const bool uniform = __ballot(active && a != a_first) == 0;  // one accession: the first active lane adds for all
    unsigned long long v[kVals];
    v[0] = uniform ? (unsigned long long)__builtin_popcountll(am) : 1ull;
    for (unsigned k = 1; k < kVals; ++k) {
      v[k] = active ? more[k - 1] : 0ull;
      if (uniform) v[k] = wave_sum(v[k]);
    }
    if (uniform ? lane == first : active) {
      const int s = lds_probe<kSlots>(key, kEmpty, a, (a * 2654435761u) >> kShift);
      if (s >= 0) {
        for (unsigned k = 0; k < kVals; ++k) atomicAdd(&val[k][s], v[k]);
      } else {
        for (unsigned k = 0; k < kVals; ++k) atomicAdd(&global[k][a], v[k]);
      }
    }
  }

  // One global add per occupied slot and sum, and the counter.
  __device__ __forceinline__ void flush(unsigned long long* const* global, unsigned long long* miss_counter) {
    __syncthreads();
    for (unsigned s = threadIdx.x; s < kSlots; s += kThreads) {
      const uint32_t k = key[s];
      if (k != kEmpty && val[0][s]) {
        for (unsigned v = 0; v < kVals; ++v) atomicAdd(&global[v][k], val[v][s]);
      }
    }
    if (threadIdx.x == 0 && miss) atomicAdd(miss_counter, miss);
  }
};

// Lane l of the wavefront brings len items (T: uint32_t or a 64-bit type, the sum of the 64 lengths must fit).  Items are numbered
// lane by lane, 0 to total - 1.  The whole wavefront constructs it and calls find() together (both shuffle).
template <class T> struct WaveList {
  T len, incl, total;
  struct Item {
    int lane;    // the lane that brought item j
    T at, len;   // j is that lane's item `at` of `len`
  };
  __device__ __forceinline__ explicit WaveList(T n) : len(n), incl(n) {
    const unsigned lane = threadIdx.x & 63u;
    for (int d = 1; d < 64; d <<= 1) {
      const T up = __shfl_up(incl, d, 64);
      if (lane >= (unsigned)d) incl += up;
    }
    total = __shfl(incl, 63, 64);
  }
  // (each lane asks for its own j; for j >= total the answer means nothing)
  __device__ __forceinline__ Item find(T j) const {
    int lo = 0, hi = 63;  // the first lane whose inclusive sum is above j
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const T v = __shfl(incl, mid, 64);  // (__shfl reads another lane's value by index: each lane its own mid)
      if (v > j) hi = mid; else lo = mid + 1;
    }
    const T o_incl = __shfl(incl, lo, 64), o_len = __shfl(len, lo, 64);
    return Item{lo, j - (o_incl - o_len), o_len};
  }
};

// t[i] = carry + t[0] + .. + t[i - 1] for i < n, in place; returns carry + all of them (in every thread).  For ONE workgroup of
// kThreads threads, every thread of which calls it; a step takes kPer consecutive elements per thread.
template <class T, unsigned kThreads, unsigned kPer> __device__ __forceinline__ T block_scan_excl(T* __restrict__ t, uint64_t n, T carry) {
  __shared__ T s_w[kThreads / 64];
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (uint64_t base = 0; base < n; base += (uint64_t)kPer * kThreads) {
    const uint64_t i = base + (uint64_t)kPer * threadIdx.x;
    T v[kPer], tot = 0;
    for (unsigned k = 0; k < kPer; ++k) {
      v[k] = i + k < n ? t[i + k] : 0;
      tot += v[k];
    }
    T incl = tot;
    for (int d = 1; d < 64; d <<= 1) {
      const T up = __shfl_up(incl, d, 64);
      if (lane >= (unsigned)d) incl += up;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (unsigned w = 0; w < kThreads / 64; ++w) {
      const T x = s_w[w];
      if (w < wv) before += x;
      all += x;
    }
    T ex = carry + before + incl - tot;
    for (unsigned k = 0; k < kPer; ++k) {
      if (i + k < n) t[i + k] = ex;
      ex += v[k];
    }
    carry += all;
    __syncthreads();  // (s_w is written again in the next step)
  }
  return carry;
}

}  // namespace mg
