// mg_identity.hip — alignment identity per accession (--identity; metalign_amd/identity.py is the definition).
//
// Per accession three sums (scored alignments, their aligned columns, their edits) and a histogram of 1001 bins of per-alignment
// identity, all u64.  One kernel:
//
//   k_ident_add   records + edits -> the sums and bins of every counting, scored record, the unscored counted.  Persistent
//                 grid-stride, one record per lane.  The load is the worst case for global atomics: most records of a sample hit a
//                 handful of accessions and a few dozen bins near 1000, so plain adds pile onto a few cache lines.  As k_cov_add:
//                 * (accession, bin) -> a hashed LDS table of 32-bit counts; accession -> a second one with the three 64-bit sums;
//                 * lanes of a wavefront that share a key add once: the sums when the wavefront's scored records share one
//                   accession, the bins by up to kRounds elected leaders (a ballot each), the rest one by one;
//                 * a key that finds no slot within kProbe adds to memory directly;
//                 * one global add per occupied slot when the workgroup ends.
//                 A launch takes at most 2^31 records, so no 32-bit count can wrap.
//   k_ident_rows  the histogram rows a caller asks for, gathered for one download.
#include "mg_internal.h"
#include "mg_identity_core.h"

using namespace mg;

struct mg_identity {
  unsigned long long* hist = nullptr;  // u64[nacc * 1001] (its own allocation, as the coverage bitmap)
  uint32_t nacc = 0;
  DevBuf sums;  // u64[3 nacc + 1]: alignments, columns, edits, unscored
  ~mg_identity() { if (hist) (void)hipFree(hist); }
};

namespace {

constexpr unsigned kBlock = 256, kHistSlots = 2048, kAccSlots = 512, kProbe = 8, kRounds = 4;
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kEmptyAcc = 0xffffffffu;
constexpr uint64_t kLaunchMax = 1ull << 31;
#ifdef MG_IDENT_NO_LDS  // (measurements only: every scored record adds to memory directly)
constexpr bool kUseLds = false;
#else
constexpr bool kUseLds = true;
#endif

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kBlock) void k_ident_add(const mg_aln_rec* __restrict__ recs, const mg_aln_edit* __restrict__ edit, uint64_t n,
                                                      double pct_id, uint32_t nacc, unsigned long long* __restrict__ hist,
                                                      unsigned long long* __restrict__ aln, unsigned long long* __restrict__ cols,
                                                      unsigned long long* __restrict__ eds, unsigned long long* __restrict__ unscored) {
  __shared__ unsigned long long s_hkey[kHistSlots];
  __shared__ uint32_t s_hcnt[kHistSlots];
  __shared__ uint32_t s_akey[kAccSlots];
  __shared__ unsigned long long s_acnt[kAccSlots], s_acol[kAccSlots], s_aed[kAccSlots];
  __shared__ unsigned long long s_unscored;
  for (unsigned i = threadIdx.x; i < kHistSlots; i += kBlock) { s_hkey[i] = kEmptyKey; s_hcnt[i] = 0; }
  for (unsigned i = threadIdx.x; i < kAccSlots; i += kBlock) { s_akey[i] = kEmptyAcc; s_acnt[i] = 0; s_acol[i] = 0; s_aed[i] = 0; }
  if (threadIdx.x == 0) s_unscored = 0;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u;
  // (no workgroup barrier inside the loop: a wavefront works on its own 64 records)
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    bool scored = false, uns = false;
    uint32_t a = 0, c = 0, e = 0;
    unsigned long long key = 0;  // a * 1001 + bin: the bin's index in hist (a < nacc)
    if (i < n) {
      const mg_aln_rec r = recs[i];
      if (mgv::counts(r, pct_id)) {
        const mg_aln_edit ed = edit[i];
        a = r.ref_new & MG_REC_REF_MASK;
        if (ed.nm != mgi::kNone && ed.cols != 0 && a < nacc) {
          scored = true;
          c = ed.cols;
          e = mgi::edits_of(ed.nm, ed.cols);
          key = (unsigned long long)a * mgi::kBins + mgi::bin_of(e, c);
        } else {
          uns = true;
        }
      }
    }
    // the unscored: one LDS add per wavefront
    const unsigned long long um = __ballot(uns);
    if (um && lane == (unsigned)__builtin_ctzll(um)) atomicAdd(&s_unscored, (unsigned long long)__builtin_popcountll(um));
    const unsigned long long sm = __ballot(scored);
    if (!sm) continue;  // (uniform over the wavefront)
    if (!kUseLds) {
      if (scored) {
        atomicAdd(&aln[a], 1ull);
        atomicAdd(&cols[a], (unsigned long long)c);
        atomicAdd(&eds[a], (unsigned long long)e);
        atomicAdd(&hist[key], 1ull);
      }
      continue;
    }
    // alignments, columns and edits per accession
    {
      const unsigned first = (unsigned)__builtin_ctzll(sm);
      const uint32_t a_first = __shfl(a, (int)first, 64);
      const bool uniform = __ballot(scored && a != a_first) == 0;
      unsigned long long add_cnt = scored ? 1ull : 0ull, add_col = scored ? c : 0u, add_ed = scored ? e : 0u;
      if (uniform) {
        add_col = wave_sum(add_col);
        add_ed = wave_sum(add_ed);
        add_cnt = (unsigned long long)__builtin_popcountll(sm);
      }
      if (uniform ? lane == first : scored) {
        const uint32_t h = (a * 2654435761u) >> 23;
        bool done = false;
        for (unsigned p = 0; p < kProbe && !done; ++p) {
          const uint32_t s = (h + p) & (kAccSlots - 1);
          const uint32_t k = atomicCAS(&s_akey[s], kEmptyAcc, a);
          if (k == kEmptyAcc || k == a) {
            atomicAdd(&s_acnt[s], add_cnt);
            atomicAdd(&s_acol[s], add_col);
            atomicAdd(&s_aed[s], add_ed);
            done = true;
          }
        }
        if (!done) {
          atomicAdd(&aln[a], add_cnt);
          atomicAdd(&cols[a], add_col);
          atomicAdd(&eds[a], add_ed);
        }
      }
    }
    // the bins: leaders add for the lanes that share their key, the lanes left after kRounds add for themselves
    {
      unsigned long long rest = sm, mine_key = key;
      uint32_t mine_cnt = 0;
      for (unsigned round = 0; round < kRounds && rest; ++round) {
        const unsigned leader = (unsigned)__builtin_ctzll(rest);
        const unsigned long long k0 = __shfl(key, (int)leader, 64);
        const unsigned long long same = __ballot(scored && key == k0) & rest;
        if (lane == leader) mine_cnt = (uint32_t)__builtin_popcountll(same);
        rest &= ~same;
      }
      if ((rest >> lane) & 1ull) mine_cnt = 1;
      if (mine_cnt) {
        const uint32_t h = (uint32_t)((mine_key * 0x9e3779b97f4a7c15ull) >> 53);
        bool done = false;
        for (unsigned p = 0; p < kProbe && !done; ++p) {
          const uint32_t s = (h + p) & (kHistSlots - 1);
          const unsigned long long k = atomicCAS(&s_hkey[s], kEmptyKey, mine_key);
          if (k == kEmptyKey || k == mine_key) {
            atomicAdd(&s_hcnt[s], mine_cnt);
            done = true;
          }
        }
        if (!done) atomicAdd(&hist[mine_key], (unsigned long long)mine_cnt);
      }
    }
  }
  __syncthreads();
  for (unsigned s = threadIdx.x; s < kHistSlots; s += kBlock) {
    const unsigned long long k = s_hkey[s];
    if (k != kEmptyKey && s_hcnt[s]) atomicAdd(&hist[k], (unsigned long long)s_hcnt[s]);
  }
  for (unsigned s = threadIdx.x; s < kAccSlots; s += kBlock) {
    const uint32_t k = s_akey[s];
    if (k != kEmptyAcc && s_acnt[s]) {
      atomicAdd(&aln[k], s_acnt[s]);
      atomicAdd(&cols[k], s_acol[s]);
      atomicAdd(&eds[k], s_aed[s]);
    }
  }
  if (threadIdx.x == 0 && s_unscored) atomicAdd(unscored, s_unscored);
}

// out[r * 1001 + b] = hist[rows[r] * 1001 + b]
__global__ __launch_bounds__(kBlock) void k_ident_rows(const unsigned long long* __restrict__ hist, const uint32_t* __restrict__ rows,
                                                       uint64_t total, unsigned long long* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint64_t r = t / mgi::kBins, b = t - r * mgi::kBins;
    out[t] = hist[(uint64_t)rows[r] * mgi::kBins + b];
  }
}

}  // namespace

extern "C" {

int mg_identity_create(uint32_t nacc, mg_identity** out) {
  MG_REQUIRE_READY();
  if (!out || nacc > MG_REC_REF_MASK) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  hipStream_t st = ctx().stream;
  std::unique_ptr<mg_identity> h(new mg_identity());
  h->nacc = nacc;
  const uint64_t hist_bytes = (uint64_t)nacc * mgi::kBins * sizeof(uint64_t), sums_bytes = (3ull * nacc + 1) * sizeof(uint64_t);
  MG_TRY(h->sums.alloc(sums_bytes));
  hipError_t e = hipMalloc((void**)&h->hist, hist_bytes + 16);
  if (e != hipSuccess) {  // (as mg_coverage_create: the allocator's cached blocks back to the runtime, once)
    (void)hipGetLastError();
    h->hist = nullptr;
    (void)hipStreamSynchronize(st);
    pool_release_all();
    e = hipMalloc((void**)&h->hist, hist_bytes + 16);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    h->hist = nullptr;
    return fail(MG_ERR_NOMEM, "the identity histograms (%llu bytes, 1001 bins of 8 bytes per accession) do not fit: %s",
                (unsigned long long)(hist_bytes + sums_bytes), hipGetErrorString(e));
  }
  MG_HIP(hipMemsetAsync(h->hist, 0, hist_bytes + 16, st));
  MG_HIP(hipMemsetAsync(h->sums.p, 0, sums_bytes, st));
  MG_HIP(hipStreamSynchronize(st));
  *out = h.release();
  return MG_OK;
}

int mg_identity_add_dev(mg_identity* h, const mg_aln_rec* d_recs, const mg_aln_edit* d_edit, uint64_t n, double pct_id) {
  MG_REQUIRE_READY();
  if (!h || (n && (!d_recs || !d_edit))) return fail(MG_ERR_ARG, "null argument");
  if (n == 0) return MG_OK;
  ProfScope ps("ident_add");
  unsigned long long* sums = h->sums.as<unsigned long long>();
  for (uint64_t at = 0; at < n; at += kLaunchMax) {
    const uint64_t m = n - at < kLaunchMax ? n - at : kLaunchMax;
    const unsigned grid = grid_cap(grid_for(m, kBlock, (unsigned)ctx().num_cus * 8), "ident_grid");
    hipLaunchKernelGGL(k_ident_add, dim3(grid), dim3(kBlock), 0, ctx().stream, d_recs + at, d_edit + at, m, pct_id, h->nacc, h->hist, sums,
                       sums + h->nacc, sums + 2ull * h->nacc, sums + 3ull * h->nacc);
    MG_HIP(hipGetLastError());
  }
  return MG_OK;
}

int mg_identity_result(mg_identity* h, uint64_t* alignments, uint64_t* columns, uint64_t* edits, uint64_t* unscored) {
  MG_REQUIRE_READY();
  if (!h || !unscored || (h->nacc && (!alignments || !columns || !edits))) return fail(MG_ERR_ARG, "null argument");
  hipStream_t st = ctx().stream;
  const uint64_t nacc = h->nacc;
  std::vector<uint64_t> s(3 * nacc + 1);
  MG_HIP(hipMemcpyAsync(s.data(), h->sums.p, s.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));
  for (uint64_t a = 0; a < nacc; ++a) {
    alignments[a] = s[a];
    columns[a] = s[nacc + a];
    edits[a] = s[2 * nacc + a];
  }
  *unscored = s[3 * nacc];
  return MG_OK;
}

int mg_identity_fetch_hist(mg_identity* h, const uint32_t* rows, uint32_t nrows, uint64_t* hist) {
  MG_REQUIRE_READY();
  if (!h || (nrows && (!rows || !hist))) return fail(MG_ERR_ARG, "null argument");
  for (uint32_t r = 0; r < nrows; ++r)
    if (rows[r] >= h->nacc) return fail(MG_ERR_ARG, "row %u: accession %u of %u", r, rows[r], h->nacc);
  if (nrows == 0) return MG_OK;
  hipStream_t st = ctx().stream;
  const uint64_t total = (uint64_t)nrows * mgi::kBins;
  DevBuf d_rows, d_out;
  MG_TRY(d_rows.alloc((uint64_t)nrows * sizeof(uint32_t)));
  MG_TRY(d_out.alloc(total * sizeof(uint64_t)));
  MG_HIP(hipMemcpyAsync(d_rows.p, rows, (uint64_t)nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_ident_rows, dim3(grid_for(total, kBlock, (unsigned)ctx().num_cus * 8)), dim3(kBlock), 0, st, h->hist,
                     d_rows.as<uint32_t>(), total, d_out.as<unsigned long long>());
  MG_HIP(hipGetLastError());
  MG_HIP(hipMemcpyAsync(hist, d_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));
  return MG_OK;
}

void mg_identity_free(mg_identity* h) { delete h; }

}  // extern "C"
