// mg_identity.hip — alignment identity per accession (--identity; metalign_amd/identity.py is the definition).
//
// Per accession three sums (scored alignments, their aligned columns, their edits) and a histogram of 1001 bins of per-alignment
// identity, all u64.  One kernel:
//
//   k_ident_add   records + edits -> the sums and bins of every counting, scored record, the unscored counted.  Persistent
//                 grid-stride, one record per lane.  The load is the worst case for global atomics: most records of a sample hit a
//                 handful of accessions and a few dozen bins near 1000, so plain adds pile onto a few cache lines.
//                 * accession -> the three 64-bit sums in hashed LDS bins (mg_side_dev.h: AccBins);
//                 * (accession, bin) -> a second hashed LDS table, of 32-bit counts, kept here (it has this one user): lanes of a
//                   wavefront that share a key add once, by up to kRounds elected leaders (a ballot each), the rest one by one; a
//                   key that finds no slot within kProbe (mg_side_dev.h: lds_probe) adds to memory directly; one global add per
//                   occupied slot when the workgroup ends.
//                 A launch takes at most 2^31 records, so no 32-bit count can wrap.
//   k_ident_rows  the histogram rows a caller asks for, gathered for one download.
#include "mg_internal.h"
#include "mg_identity_core.h"
#include "mg_side_dev.h"

using namespace mg;

struct mg_identity {
  unsigned long long* hist = nullptr;  // u64[nacc * 1001] (its own allocation, as the coverage bitmap)
  uint32_t nacc = 0;
  DevBuf sums;  // u64[3 nacc + 1]: alignments, columns, edits, unscored
  ~mg_identity() { if (hist) (void)hipFree(hist); }
};

namespace {

constexpr unsigned kBlock = 256, kHistSlots = 2048, kAccSlots = 512, kRounds = 4;
constexpr unsigned long long kEmptyKey = ~0ull;
#ifdef MG_IDENT_NO_LDS  // (measurements only: every scored record adds to memory directly)
constexpr bool kUseLds = false;
#else
constexpr bool kUseLds = true;
#endif

__global__ __launch_bounds__(kBlock) void k_ident_add(const mg_aln_rec* __restrict__ recs, const mg_aln_edit* __restrict__ edit, uint64_t n,
                                                      double pct_id, uint32_t nacc, unsigned long long* __restrict__ hist,
                                                      unsigned long long* __restrict__ aln, unsigned long long* __restrict__ cols,
                                                      unsigned long long* __restrict__ eds, unsigned long long* __restrict__ unscored) {
  // (ONE object: on their own the bins, 8 bytes short of a multiple of 16, would cost the workgroup 8 bytes of padding)
  __shared__ struct {
    unsigned long long hkey[kHistSlots];
    uint32_t hcnt[kHistSlots];
    AccBins<kAccSlots, 3, kBlock> acc;
  } s_lds;
  unsigned long long* const s_hkey = s_lds.hkey;
  uint32_t* const s_hcnt = s_lds.hcnt;
  auto& bins = s_lds.acc;
  unsigned long long* const sums[3] = {aln, cols, eds};
  for (unsigned i = threadIdx.x; i < kHistSlots; i += kBlock) { s_hkey[i] = kEmptyKey; s_hcnt[i] = 0; }
  bins.init();  // (and the barrier behind both tables)
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
    bins.count_one(uns);
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
    const unsigned long long col_ed[2] = {c, e};
    bins.add(scored, a, col_ed, sums);
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
        const int s = lds_probe<kHistSlots, kProbe>(s_hkey, kEmptyKey, mine_key, (uint32_t)((mine_key * 0x9e3779b97f4a7c15ull) >> 53));
        if (s >= 0) atomicAdd(&s_hcnt[s], mine_cnt);
        else atomicAdd(&hist[mine_key], (unsigned long long)mine_cnt);
      }
    }
  }
  bins.flush(sums, unscored);  // (behind the barrier that ends the loop for both tables)
  for (unsigned s = threadIdx.x; s < kHistSlots; s += kBlock) {
    const unsigned long long k = s_hkey[s];
    if (k != kEmptyKey && s_hcnt[s]) atomicAdd(&hist[k], (unsigned long long)s_hcnt[s]);
  }
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
  MG_TRY(own_alloc((void**)&h->hist, hist_bytes + 16,
                   "the identity histograms (%llu bytes, 1001 bins of 8 bytes per accession) do not fit: %s", hist_bytes + sums_bytes));
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
    hipLaunchKernelGGL(k_ident_add, dim3(side_grid(m, kBlock, "ident_grid")), dim3(kBlock), 0, ctx().stream, d_recs + at, d_edit + at, m,
                       pct_id, h->nacc, h->hist, sums, sums + h->nacc, sums + 2ull * h->nacc, sums + 3ull * h->nacc);
    MG_HIP(hipGetLastError());
  }
  return MG_OK;
}

int mg_identity_result(mg_identity* h, uint64_t* alignments, uint64_t* columns, uint64_t* edits, uint64_t* unscored) {
  MG_REQUIRE_READY();
  if (!h || !unscored || (h->nacc && (!alignments || !columns || !edits))) return fail(MG_ERR_ARG, "null argument");
  uint64_t* const out[3] = {alignments, columns, edits};
  return fetch_sums(h->sums.p, h->nacc, out, 3, unscored);
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
