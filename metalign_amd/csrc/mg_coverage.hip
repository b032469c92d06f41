// mg_coverage.hip — breadth and depth of coverage per accession (--coverage; metalign_amd/coverage.py is the definition).
//
// One bit per reference base, every accession on a 32-bit word boundary at a 64-bit word offset.  Two kernels:
//
//   k_cov_add     records + places -> the bits of every counting, placed record's interval ORed in, the accession's alignments and
//                 aligned bases summed, the unplaced counted.
//                 * The work per record varies from 3 words (a short read) to 2^15 and more (an assembly): every wavefront
//                   flattens the word lists of its 64 records (an inclusive scan of the words per record) and its lanes stride
//                   the total, so neighbouring lanes take neighbouring words of a long record and no lane walks one alone.
//                 * Bits are only ever set: a relaxed load that finds them set skips the atomic (a stale load costs one atomic
//                   that was not needed).  At depth 40 that is most of them.
//                 * Most records of a sample hit a few accessions: the sums go to hashed LDS bins.
//   k_cov_count   the set bits per accession: every wavefront takes blocks of kCountWords words, finds the accession of its
//                 first word in the offsets, and gives one 64-bit add per block and accession.
// The flattened list, the bins and the wavefront's sum are mg_side_dev.h's (WaveList, AccBins, wave_sum).
#include "mg_internal.h"
#include "mg_coverage_core.h"
#include "mg_side_dev.h"

using namespace mg;

struct mg_coverage {
  uint32_t* bits = nullptr;  // u32[nwords] (its own allocation: up to gigabytes, not worth a size class's slack in the pool)
  uint64_t nwords = 0;
  uint32_t nacc = 0;
  DevBuf off;   // u64[nacc + 1]: accession a's first word
  DevBuf len;   // u64[nacc]
  DevBuf sums;  // u64[3 nacc + 1]: alignments, aligned_bases, covered_bases, unplaced
  ~mg_coverage() { if (bits) (void)hipFree(bits); }
};

namespace {

constexpr unsigned kCovBlock = 256, kCovBins = 1024;
constexpr uint64_t kCountWords = 1024;  // per wavefront and step of k_cov_count

__global__ __launch_bounds__(kCovBlock) void k_cov_add(const mg_aln_rec* __restrict__ recs, const mg_aln_place* __restrict__ place,
                                                       uint64_t n, double pct_id, const uint64_t* __restrict__ len,
                                                       const uint64_t* __restrict__ off, uint32_t nacc, uint32_t* __restrict__ bits,
                                                       unsigned long long* __restrict__ aln, unsigned long long* __restrict__ bases,
                                                       unsigned long long* __restrict__ unplaced) {
  __shared__ AccBins<kCovBins, 2, kCovBlock> bins;
  unsigned long long* const sums[2] = {aln, bases};
  bins.init();
  const unsigned lane = threadIdx.x & 63u;
  // (no workgroup barrier inside the loop: a wavefront works on its own 64 records)
  for (uint64_t base = (uint64_t)blockIdx.x * kCovBlock; base < n; base += (uint64_t)gridDim.x * kCovBlock) {
    const uint64_t i = base + threadIdx.x;
    uint32_t a = 0, m0 = 0, m1 = 0;
    unsigned long long clen = 0, gw0 = 0, nw = 0;
    bool unp = false;
    if (i < n) {
      const mg_aln_rec r = recs[i];
      if (mgv::counts(r, pct_id)) {
        const mg_aln_place pl = place[i];
        a = r.ref_new & MG_REC_REF_MASK;
        clen = a < nacc ? mgv::clipped(pl.pos0, pl.span, len[a]) : 0;
        if (clen) {
          uint64_t w0, w1;
          mgv::interval(pl.pos0, pl.pos0 + clen, &w0, &m0, &w1, &m1);
          nw = w1 - w0 + 1;
          gw0 = off[a] + w0;
        } else {
          unp = true;
        }
      }
    }
    bins.count_one(unp);                  // the unplaced
    bins.add(clen != 0, a, &clen, sums);  // alignments and aligned bases
    // the bits: the wavefront's flattened word list, its lanes striding it
    const WaveList<unsigned long long> words(nw);
    for (unsigned long long j0 = 0; j0 < words.total; j0 += 64) {  // (uniform: every lane takes part in the shuffles)
      const unsigned long long j = j0 + lane;
      const auto it = words.find(j);
      const unsigned long long r_gw0 = __shfl(gw0, it.lane, 64);
      const uint32_t r_m0 = __shfl(m0, it.lane, 64), r_m1 = __shfl(m1, it.lane, 64);
      if (j < words.total) {
        uint32_t mask = 0xffffffffu;
        if (it.at == 0) mask &= r_m0;
        if (it.at == it.len - 1) mask &= r_m1;
        uint32_t* w = bits + (r_gw0 + it.at);
        const uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & mask) != mask) (void)__hip_atomic_fetch_or(w, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  bins.flush(sums, unplaced);
}

__global__ __launch_bounds__(kCovBlock) void k_cov_count(const uint32_t* __restrict__ bits, uint64_t nwords,
                                                         const uint64_t* __restrict__ off, uint32_t nacc,
                                                         unsigned long long* __restrict__ cov) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kCovBlock / 64) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (kCovBlock / 64);
  for (uint64_t t0 = wave * kCountWords; t0 < nwords; t0 += nwaves * kCountWords) {
    const uint64_t t1 = t0 + kCountWords < nwords ? t0 + kCountWords : nwords;
    uint32_t a = mgv::owner_of(off, nacc, t0);  // (off[nacc] = nwords > t0)
    uint64_t s = t0;
    while (s < t1) {
      const uint64_t e = off[a + 1] < t1 ? off[a + 1] : t1;
      unsigned long long sum = 0;
      for (uint64_t w = s + lane; w < e; w += 64) sum += (unsigned long long)__builtin_popcount(bits[w]);
      sum = wave_sum(sum);
      if (lane == 0 && sum) atomicAdd(&cov[a], sum);
      s = e;
      a = mgv::owner_from(off, nacc, a, s);  // (over the accessions without words)
    }
  }
}

}  // namespace

extern "C" {

int mg_coverage_create(const uint64_t* lengths, uint32_t nacc, mg_coverage** out) {
  MG_REQUIRE_READY();
  if (!out || (nacc && !lengths) || nacc > MG_REC_REF_MASK) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  hipStream_t st = ctx().stream;
  std::unique_ptr<mg_coverage> c(new mg_coverage());
  c->nacc = nacc;
  std::vector<uint64_t> h_off(nacc + 1ull, 0);
  for (uint32_t a = 0; a < nacc; ++a) {
    if (lengths[a] >> 48) return fail(MG_ERR_ARG, "accession %u: length %llu", a, (unsigned long long)lengths[a]);
    h_off[a + 1] = h_off[a] + (lengths[a] + 31) / 32;
  }
  c->nwords = h_off[nacc];
  MG_TRY(c->off.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(c->len.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(c->sums.alloc((3ull * nacc + 1) * sizeof(uint64_t)));
  MG_TRY(own_alloc((void**)&c->bits, c->nwords * sizeof(uint32_t) + 16,
                   "the coverage bitmap (%llu bytes, one bit per reference base) does not fit: %s", c->nwords * sizeof(uint32_t)));
  MG_HIP(hipMemsetAsync(c->bits, 0, c->nwords * sizeof(uint32_t) + 16, st));
  MG_HIP(hipMemsetAsync(c->sums.p, 0, (3ull * nacc + 1) * sizeof(uint64_t), st));
  MG_HIP(hipMemcpyAsync(c->off.p, h_off.data(), (nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (nacc) MG_HIP(hipMemcpyAsync(c->len.p, lengths, (uint64_t)nacc * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipStreamSynchronize(st));  // (h_off and the caller's lengths are free from here)
  *out = c.release();
  return MG_OK;
}

int mg_coverage_add_dev(mg_coverage* c, const mg_aln_rec* d_recs, const mg_aln_place* d_place, uint64_t n, double pct_id) {
  MG_REQUIRE_READY();
  if (!c || (n && (!d_recs || !d_place))) return fail(MG_ERR_ARG, "null argument");
  if (n == 0) return MG_OK;
  ProfScope ps("cov_add");
  unsigned long long* sums = c->sums.as<unsigned long long>();
  hipLaunchKernelGGL(k_cov_add, dim3(side_grid(n, kCovBlock, "cov_grid")), dim3(kCovBlock), 0, ctx().stream, d_recs, d_place, n, pct_id, c->len.as<uint64_t>(),
                     c->off.as<uint64_t>(), c->nacc, c->bits, sums, sums + c->nacc, sums + 3ull * c->nacc);
  MG_HIP(hipGetLastError());
  return MG_OK;
}

int mg_coverage_result(mg_coverage* c, uint64_t* alignments, uint64_t* aligned_bases, uint64_t* covered_bases, uint64_t* unplaced) {
  MG_REQUIRE_READY();
  if (!c || !unplaced || (c->nacc && (!alignments || !aligned_bases || !covered_bases))) return fail(MG_ERR_ARG, "null argument");
  hipStream_t st = ctx().stream;
  const uint64_t nacc = c->nacc;
  unsigned long long* sums = c->sums.as<unsigned long long>();
  if (nacc) MG_HIP(hipMemsetAsync(sums + 2 * nacc, 0, nacc * sizeof(uint64_t), st));
  if (c->nwords) {
    ProfScope ps("cov_count");
    const uint64_t steps = (c->nwords + kCountWords - 1) / kCountWords;
    hipLaunchKernelGGL(k_cov_count, dim3(side_grid(steps, kCovBlock / 64, "cov_grid")), dim3(kCovBlock), 0, st, c->bits, c->nwords,
                       c->off.as<uint64_t>(), c->nacc, sums + 2 * nacc);
    MG_HIP(hipGetLastError());
  }
  uint64_t* const out[3] = {alignments, aligned_bases, covered_bases};
  return fetch_sums(sums, nacc, out, 3, unplaced);
}

void mg_coverage_free(mg_coverage* c) { delete c; }

}  // extern "C"
