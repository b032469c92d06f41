// mg_variants.hip — per-site allele counts and strain diversity per accession (--variants, --variant_sites;
// metalign_amd/variants.py is the definition, mg_variants_core.h the per-site rule).
//
// Four u32 per reference base (the reads' A, C, G and T there), every accession at a 64-bit site offset.  Three kernels, one of
// them in two forms:
//
//   k_var_add           records + entries + pool -> one add per code below 4 of every counting, piled record, clipped at the
//                       accession's length; the accession's alignments and the unpiled counted in hashed LDS bins (mg_side_dev.h:
//                       AccBins).  Persistent grid-stride.  The work per record is its span — 150 for a short read, 2^21 - 1 at
//                       most — so every wavefront flattens the base lists of its 64 records (mg_side_dev.h: WaveList, an inclusive
//                       scan of the clipped spans) and its lanes stride the total: neighbouring lanes take
//                       neighbouring bases of one record, that is neighbouring 16-byte cells and the same or neighbouring pool bytes,
//                       and no lane walks a long record alone.  The adds return nothing.
//   k_var_sites<false>  the sums: every wavefront takes blocks of kStep sites, finds the accession of its first site in the offsets
//                       (mgv::owner_of) and judges the sites of accessions that have an alignment: callable, polymorphic, pairs and
//                       discordant summed over the wavefront, one 64-bit add per block, accession and sum; the block's polymorphic
//                       sites counted.
//   k_var_scan          the exclusive scan of the blocks' counts by ONE workgroup (mg_side_dev.h: block_scan_excl): nobody waits
//                       for another workgroup.
//   k_var_sites<true>   the sites: the same walk a second time; a polymorphic site goes to the block's base + the polymorphic sites
//                       before it in the block (a ballot and mbcnt per 64 sites), so the sites come out ordered by (accession row,
//                       pos0) whatever the grid.
//   k_var_diff<...>     the same two passes against the reference code of every site (mg_variants_diff; --ani, --vcf): compared,
//                       con_subs, pop_subs and ref_other per accession, and the sites where the sample differs from the reference.
//                       The walk exists once (var_walk): k_var_sites and k_var_diff instantiate it with their pass.
//   k_var_consensus     the counts of a list of accession rows -> their consensus sequences as text (--consensus;
//                       metalign_amd/consensus.py is the definition), laid out over OUTPUT bytes: every wavefront takes kTextStep
//                       bytes of the texts, which lie back to back, finds the row of its first byte in the text offsets
//                       (mgv::owner_of, every lane then mgv::owner_from for its own byte) and each lane judges the site its byte
//                       shows (mgvar::text_at, mgvar::consensus_char): neighbouring lanes load neighbouring 16-byte cells, four
//                       lanes' characters are packed into one dword store.  Reads the counts only.
#include "mg_internal.h"
#include "mg_variants_core.h"
#include "mg_side_dev.h"

using namespace mg;

struct mg_variants {
  uint32_t* cnt = nullptr;  // u32[4 * nsites] (its own allocation, as the coverage bitmap)
  uint64_t nsites = 0, nblocks = 0, npoly = 0;
  uint32_t nacc = 0;
  bool finished = false;
  DevBuf off;    // u64[nacc + 1]: accession a's first site
  DevBuf len;    // u64[nacc]
  DevBuf sums;   // u64[5 nacc + 1]: alignments, callable, polymorphic, pairs, discordant, unpiled
  DevBuf blk;    // u64[1 + nblocks]: the scan's carry, then the blocks' polymorphic sites / bases
  DevBuf sites;  // mg_variant_site[npoly]
  std::vector<uint64_t> h_len;  // the lengths again, on the host: what mg_variants_consensus sizes the texts by
  // mg_variants_diff keeps its own: finish's blocks and sites stay as they are
  DevBuf dsums;   // u64[4 nacc]: compared, con_subs, pop_subs, ref_other
  DevBuf dblk;    // u64[1 + nblocks]
  DevBuf dsites;  // mg_variant_diff[ndiff]
  uint64_t ndiff = 0;
  bool diffed = false;
  ~mg_variants() { if (cnt) (void)hipFree(cnt); }
};

namespace {

constexpr unsigned kBlock = 256, kBins = 1024, kScanBlock = 256;
constexpr uint64_t kStep = 1024;  // sites per wavefront and step of k_var_sites
constexpr uint64_t kTextStep = 1024;  // output bytes per wavefront and step of k_var_consensus (a multiple of 64)

struct PoolView {
  const uint8_t* p;
  __device__ __forceinline__ uint32_t operator[](uint64_t i) const { return p[i]; }
};

__global__ __launch_bounds__(kBlock) void k_var_add(const mg_aln_rec* __restrict__ recs, const mg_aln_bases* __restrict__ bases,
                                                    const uint8_t* __restrict__ pool, uint64_t n, double pct_id,
                                                    const uint64_t* __restrict__ len, const uint64_t* __restrict__ off, uint32_t nacc,
                                                    uint32_t* __restrict__ cnt, unsigned long long* __restrict__ aln,
                                                    unsigned long long* __restrict__ unpiled) {
  __shared__ AccBins<kBins, 1, kBlock> bins;
  unsigned long long* const sums[1] = {aln};
  bins.init();
  const unsigned lane = threadIdx.x & 63u;
  const PoolView pv{pool};
  // (no workgroup barrier inside the loop: a wavefront works on its own 64 records)
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    uint32_t a = 0, clen = 0;
    unsigned long long site0 = 0, poff = 0;
    bool unp = false;
    if (i < n) {
      const mg_aln_rec r = recs[i];
      if (mgv::counts(r, pct_id)) {
        const mg_aln_bases e = bases[i];
        a = r.ref_new & MG_REC_REF_MASK;
        // (span <= kMaxPileSpan by the entry's definition: an entry that says more is cut there, so that 64 of them sum in 32 bits)
        const uint32_t span = e.span < mgvar::kMaxPileSpan ? e.span : mgvar::kMaxPileSpan;
        clen = a < nacc ? (uint32_t)mgv::clipped(e.pos0, span, len[a]) : 0u;
        if (clen) {
          site0 = off[a] + e.pos0;
          poff = e.off;
        } else {
          unp = true;
        }
      }
    }
    bins.count_one(unp);                    // the unpiled
    bins.add(clen != 0, a, nullptr, sums);  // alignments
    // (a wavefront without a piled record skips the list's six-step scan: this kernel always had that exit and keeps it, k_cov_add
    // never had one — each stays as it was measured)
    if (!__ballot(clen != 0)) continue;  // (uniform over the wavefront)
    // the bases: the wavefront's flattened list, its lanes striding it (64 * kMaxPileSpan < 2^32)
    const WaveList<uint32_t> codes(clen);
    for (uint32_t j0 = 0; j0 < codes.total; j0 += 64) {  // (uniform: every lane takes part in the shuffles)
      const uint32_t j = j0 + lane;
      const auto it = codes.find(j);
      const unsigned long long r_site = __shfl(site0, it.lane, 64), r_poff = __shfl(poff, it.lane, 64);
      if (j < codes.total) {  // (it.at < it.len: inside the entry's codes and the accession's sites)
        const uint32_t code = mgvar::code_at(pv, r_poff, it.at);
        if (code < 4) (void)__hip_atomic_fetch_add(cnt + ((r_site + it.at) * 4 + code), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  bins.flush(sums, unpiled);
}

// Where a flagged site goes among the flagged sites of a walk: `at` + the flagged lanes below this one; `at` moves on by all of
// them.  (The whole wavefront calls it.)
__device__ __forceinline__ unsigned long long ballot_slot(bool flag, unsigned long long& at) {
  const unsigned long long pm = __ballot(flag);
  const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
  const unsigned long long o = at + below;
  at += (unsigned long long)__builtin_popcountll(pm);
  return o;
}

// THE walk over the sites, which the passes of finish (SitesPass) and of the comparison with the reference (DiffPass) share: every
// wavefront takes blocks of kStep sites, finds the accession of its first site in the offsets (mgv::owner_of) and moves on from
// there (mgv::owner_from); the sites of an accession without an alignment, or which the pass does not take, are stepped over;
// the others go to the pass 64 at a time, every lane of the wavefront calling site() so that it may ballot.  A pass is
//   takes(a)                    whether accession a's sites are looked at (beside aln[a] != 0)
//   open_block(b) / close_block(b)   around a block's sites
//   open_acc() / close_acc(a)        around the sites of one accession inside a block
//   site(a, w, in, n4)          site w of accession a (in: w is a site of the run; else n4 is 0 and the lane only takes part)
template <class Pass>
__device__ __forceinline__ void var_walk(const uint32_t* __restrict__ cnt, uint64_t nsites, uint64_t nblocks,
                                         const uint64_t* __restrict__ off, uint32_t nacc, const unsigned long long* __restrict__ aln,
                                         Pass& pass) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / 64);
  const uint4* cnt4 = reinterpret_cast<const uint4*>(cnt);
  for (uint64_t b = wave; b < nblocks; b += nwaves) {
    const uint64_t t0 = b * kStep, t1 = t0 + kStep < nsites ? t0 + kStep : nsites;
    uint32_t a = mgv::owner_of(off, nacc, t0);  // (off[nacc] = nsites > t0)
    uint64_t s = t0;
    pass.open_block(b);
    while (s < t1) {
      const uint64_t e = off[a + 1] < t1 ? off[a + 1] : t1;
      if (aln[a] && pass.takes(a)) {  // (an accession without an alignment has no count)
        pass.open_acc();
        for (uint64_t w0 = s; w0 < e; w0 += 64) {  // (uniform: every lane takes part in the ballot)
          const uint64_t w = w0 + lane;
          uint32_t n4[4] = {0, 0, 0, 0};
          if (w < e) {
            const uint4 v = cnt4[w];
            n4[0] = v.x; n4[1] = v.y; n4[2] = v.z; n4[3] = v.w;
          }
          pass.site(a, w, w < e, n4);
        }
        pass.close_acc(a);
      }
      s = e;
      a = mgv::owner_from(off, nacc, a, s);  // (over the accessions without sites)
    }
    pass.close_block(b);
  }
}

// Both passes of finish: kEmit = false sums and counts, kEmit = true writes the polymorphic sites.
template <bool kEmit> struct SitesPass {
  uint32_t min_depth, min_count, permille;
  const uint64_t* off;
  unsigned long long *callable_, *poly, *pairs, *disc, *blk;
  mg_variant_site* out;
  uint64_t nout;
  unsigned lane;
  unsigned long long at, c_call, c_poly, c_pairs, c_disc;  // at — kEmit: where the block's next polymorphic site goes; else: their count

  __device__ __forceinline__ bool takes(uint32_t) const { return true; }
  __device__ __forceinline__ void open_block(uint64_t b) { at = kEmit ? blk[b] : 0ull; }
  __device__ __forceinline__ void open_acc() { c_call = c_poly = c_pairs = c_disc = 0; }
  __device__ __forceinline__ void site(uint32_t a, uint64_t w, bool in, const uint32_t n4[4]) {
    bool is_poly = false;
    if (in) {
      const mgvar::Site st = mgvar::site_of(n4, min_depth, min_count, permille);
      is_poly = st.polymorphic;
      if (!kEmit) {
        c_call += st.callable_ ? 1u : 0u;
        c_poly += is_poly ? 1u : 0u;
        c_pairs += st.pairs;
        c_disc += st.discordant;
      }
    }
    if (kEmit) {
      const unsigned long long o = ballot_slot(is_poly, at);
      if (is_poly && o < nout) {
        mg_variant_site vs;
        vs.acc = a;
        vs.pos0 = (uint32_t)(w - off[a]);
        vs.n[0] = n4[0]; vs.n[1] = n4[1]; vs.n[2] = n4[2]; vs.n[3] = n4[3];
        out[o] = vs;
      }
    }
  }
  __device__ __forceinline__ void close_acc(uint32_t a) {
    if (kEmit) return;
    c_call = wave_sum(c_call);
    c_poly = wave_sum(c_poly);
    c_pairs = wave_sum(c_pairs);
    c_disc = wave_sum(c_disc);
    if (lane == 0) {
      if (c_call) atomicAdd(&callable_[a], c_call);
      if (c_poly) atomicAdd(&poly[a], c_poly);
      if (c_pairs) atomicAdd(&pairs[a], c_pairs);
      if (c_disc) atomicAdd(&disc[a], c_disc);
    }
    at += c_poly;
  }
  __device__ __forceinline__ void close_block(uint64_t b) {
    if (!kEmit && lane == 0) blk[b] = at;
  }
};

template <bool kEmit>
__global__ __launch_bounds__(kBlock) void k_var_sites(const uint32_t* __restrict__ cnt, uint64_t nsites, uint64_t nblocks,
                                                      const uint64_t* __restrict__ off, uint32_t nacc,
                                                      const unsigned long long* __restrict__ aln, uint32_t min_depth, uint32_t min_count,
                                                      uint32_t permille, unsigned long long* __restrict__ callable_,
                                                      unsigned long long* __restrict__ poly, unsigned long long* __restrict__ pairs,
                                                      unsigned long long* __restrict__ disc, unsigned long long* __restrict__ blk,
                                                      mg_variant_site* __restrict__ out, uint64_t nout) {
  SitesPass<kEmit> pass{min_depth, min_count, permille, off, callable_, poly, pairs, disc, blk, out, nout, threadIdx.x & 63u, 0, 0, 0, 0, 0};
  var_walk(cnt, nsites, nblocks, off, nacc, aln, pass);
}

// Both passes of the comparison with the reference (mg_variants_diff; metalign_amd/refdiff.py is the definition, mgvar::diff_of the
// per-site rule): the accessions with an alignment AND a loaded reference; a site's reference code is ref[w], one byte beside the
// sixteen of its counts.  kEmit = false sums compared, con_subs, pop_subs and ref_other per accession and counts the block's
// emitted sites; kEmit = true writes them at the block's base + their rank, so they come out ordered by (accession row, pos0).
template <bool kEmit> struct DiffPass {
  uint32_t min_depth, min_count, permille;
  const uint64_t* off;
  const uint8_t *ref, *loaded;
  unsigned long long *compared, *con, *pop, *other, *blk;
  mg_variant_diff* out;
  uint64_t nout;
  unsigned lane;
  unsigned long long at, c_cmp, c_con, c_pop, c_oth, c_emit;

  __device__ __forceinline__ bool takes(uint32_t a) const { return loaded[a] != 0; }
  __device__ __forceinline__ void open_block(uint64_t b) { at = kEmit ? blk[b] : 0ull; }
  __device__ __forceinline__ void open_acc() { c_cmp = c_con = c_pop = c_oth = c_emit = 0; }
  __device__ __forceinline__ void site(uint32_t a, uint64_t w, bool in, const uint32_t n4[4]) {
    bool emit = false;
    uint32_t r = 0;
    if (in) {
      r = ref[w];
      const mgvar::Diff d = mgvar::diff_of(n4, r, min_depth, min_count, permille);
      emit = d.emitted;
      if (!kEmit) {
        c_cmp += d.compared ? 1u : 0u;
        c_con += d.con_sub ? 1u : 0u;
        c_pop += d.pop_sub ? 1u : 0u;
        c_oth += d.ref_other ? 1u : 0u;
        c_emit += emit ? 1u : 0u;
      }
    }
    if (kEmit) {
      const unsigned long long o = ballot_slot(emit, at);
      if (emit && o < nout) {
        mg_variant_diff vd;
        vd.acc = a;
        vd.pos0 = (uint32_t)(w - off[a]);
        vd.n[0] = n4[0]; vd.n[1] = n4[1]; vd.n[2] = n4[2]; vd.n[3] = n4[3];
        vd.ref = r;
        out[o] = vd;
      }
    }
  }
  __device__ __forceinline__ void close_acc(uint32_t a) {
    if (kEmit) return;
    c_cmp = wave_sum(c_cmp);
    c_con = wave_sum(c_con);
    c_pop = wave_sum(c_pop);
    c_oth = wave_sum(c_oth);
    c_emit = wave_sum(c_emit);
    if (lane == 0) {
      if (c_cmp) atomicAdd(&compared[a], c_cmp);
      if (c_con) atomicAdd(&con[a], c_con);
      if (c_pop) atomicAdd(&pop[a], c_pop);
      if (c_oth) atomicAdd(&other[a], c_oth);
    }
    at += c_emit;
  }
  __device__ __forceinline__ void close_block(uint64_t b) {
    if (!kEmit && lane == 0) blk[b] = at;
  }
};

template <bool kEmit>
__global__ __launch_bounds__(kBlock) void k_var_diff(const uint32_t* __restrict__ cnt, uint64_t nsites, uint64_t nblocks,
                                                     const uint64_t* __restrict__ off, uint32_t nacc,
                                                     const unsigned long long* __restrict__ aln, const uint8_t* __restrict__ ref,
                                                     const uint8_t* __restrict__ loaded, uint32_t min_depth, uint32_t min_count,
                                                     uint32_t permille, unsigned long long* __restrict__ compared,
                                                     unsigned long long* __restrict__ con, unsigned long long* __restrict__ pop,
                                                     unsigned long long* __restrict__ other, unsigned long long* __restrict__ blk,
                                                     mg_variant_diff* __restrict__ out, uint64_t nout) {
  DiffPass<kEmit> pass{min_depth, min_count, permille, off, ref, loaded, compared, con, pop, other, blk, out, nout, threadIdx.x & 63u,
                       0, 0, 0, 0, 0, 0};
  var_walk(cnt, nsites, nblocks, off, nacc, aln, pass);
}

// t[i] = the counts before block i; *total = all of them
__global__ __launch_bounds__(kScanBlock) void k_var_scan(unsigned long long* __restrict__ t, uint64_t nblocks,
                                                         unsigned long long* __restrict__ total) {
  const unsigned long long all = block_scan_excl<unsigned long long, kScanBlock, 1>(t, nblocks, 0ull);
  if (threadIdx.x == 0) *total = all;
}

// The texts of rows[0 .. nrows) back to back: toff[r] is the first byte of row r's text, toff[nrows] = total their sum.  Byte i of
// the buffer belongs to the row that owns offset i; a row of length 0 has no byte and owns nothing.  out32 has (total + 3) / 4 words;
// the bytes of the last word behind `total` are written as 0.
__global__ __launch_bounds__(kBlock) void k_var_consensus(const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                                          const uint64_t* __restrict__ len, const uint64_t* __restrict__ toff,
                                                          const uint32_t* __restrict__ rows, uint32_t nrows, uint64_t total,
                                                          uint64_t nsteps, uint32_t min_depth, uint32_t min_count, uint32_t permille,
                                                          uint32_t iupac, uint32_t width, uint32_t* __restrict__ out32) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / 64);
  const uint4* cnt4 = reinterpret_cast<const uint4*>(cnt);
  for (uint64_t b = wave; b < nsteps; b += nwaves) {
    const uint64_t t0 = b * kTextStep, t1 = t0 + kTextStep < total ? t0 + kTextStep : total;
    uint32_t r = mgv::owner_of(toff, nrows, t0);  // (toff[nrows] = total > t0)
    for (uint64_t i0 = t0; i0 < t1; i0 += 64) {    // (uniform: every lane takes part in the shuffles; i0 is a multiple of 64)
      const uint64_t i = i0 + lane;
      uint32_t ch = 0;
      if (i < total) {
        r = mgv::owner_from(toff, nrows, r, i);  // (the lane's own row: r < nrows, as i < toff[nrows])
        const uint32_t a = rows[r];
        // (i - toff[r] < text_bytes(len[a]): a byte that is no newline shows a site below len[a], a cell of accession a)
        const mgvar::TextAt t = mgvar::text_at(i - toff[r], width, len[a]);
        ch = '\n';
        if (!t.newline) {
          const uint4 v = cnt4[off[a] + t.site];
          const uint32_t n4[4] = {v.x, v.y, v.z, v.w};
          ch = mgvar::consensus_char(n4, min_depth, min_count, permille, iupac != 0);
        }
      }
      // lanes 4q .. 4q + 3 hold bytes 4q .. 4q + 3 of a word: lane 4q stores it
      uint32_t w = ch | ((uint32_t)__shfl_down(ch, 1, 64) << 8);
      w |= (uint32_t)__shfl_down(w, 2, 64) << 16;
      if ((lane & 3u) == 0 && i < total) out32[i >> 2] = w;
    }
  }
}

unsigned var_grid(uint64_t items, unsigned per_block) { return side_grid(items, per_block, "var_grid"); }

}  // namespace

extern "C" {

int mg_variants_create(const uint64_t* lengths, uint32_t nacc, mg_variants** out) {
  MG_REQUIRE_READY();
  if (!out || (nacc && !lengths) || nacc > MG_REC_REF_MASK) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  hipStream_t st = ctx().stream;
  std::unique_ptr<mg_variants> h(new mg_variants());
  h->nacc = nacc;
  std::vector<uint64_t> h_off(nacc + 1ull, 0);
  for (uint32_t a = 0; a < nacc; ++a) {
    if (lengths[a] >> 48) return fail(MG_ERR_ARG, "accession %u: length %llu", a, (unsigned long long)lengths[a]);
    h_off[a + 1] = h_off[a] + lengths[a];
  }
  h->nsites = h_off[nacc];
  h->nblocks = (h->nsites + kStep - 1) / kStep;
  MG_TRY(h->off.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(h->len.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(h->sums.alloc((5ull * nacc + 1) * sizeof(uint64_t)));
  MG_TRY(h->blk.alloc((h->nblocks + 1) * sizeof(uint64_t)));
  const uint64_t bytes = h->nsites * 16 + 16;
  MG_TRY(own_alloc((void**)&h->cnt, bytes, "the allele counts (%llu bytes, sixteen per reference base) do not fit: %s", bytes));
  MG_HIP(hipMemsetAsync(h->cnt, 0, bytes, st));
  MG_HIP(hipMemsetAsync(h->sums.p, 0, (5ull * nacc + 1) * sizeof(uint64_t), st));
  MG_HIP(hipMemcpyAsync(h->off.p, h_off.data(), (nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (nacc) MG_HIP(hipMemcpyAsync(h->len.p, lengths, (uint64_t)nacc * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  h->h_len.assign(lengths, lengths + nacc);
  MG_HIP(hipStreamSynchronize(st));  // (h_off and the caller's lengths are free from here)
  *out = h.release();
  return MG_OK;
}

int mg_variants_add_dev(mg_variants* h, const mg_aln_rec* d_recs, const mg_aln_bases* d_bases, const uint8_t* d_pool, uint64_t n,
                        double pct_id) {
  MG_REQUIRE_READY();
  if (!h || (n && (!d_recs || !d_bases))) return fail(MG_ERR_ARG, "null argument");
  if (n == 0) return MG_OK;
  ProfScope ps("var_add");
  unsigned long long* sums = h->sums.as<unsigned long long>();
  for (uint64_t at = 0; at < n; at += kLaunchMax) {
    const uint64_t m = n - at < kLaunchMax ? n - at : kLaunchMax;
    hipLaunchKernelGGL(k_var_add, dim3(var_grid(m, kBlock)), dim3(kBlock), 0, ctx().stream, d_recs + at, d_bases + at, d_pool, m, pct_id,
                       h->len.as<uint64_t>(), h->off.as<uint64_t>(), h->nacc, h->cnt, sums, sums + 5ull * h->nacc);
    MG_HIP(hipGetLastError());
  }
  return MG_OK;
}

int mg_variants_finish(mg_variants* h, uint32_t min_depth, uint32_t min_count, uint32_t freq_permille, uint64_t* alignments,
                       uint64_t* callable_sites, uint64_t* polymorphic_sites, uint64_t* pairs, uint64_t* discordant, uint64_t* unpiled,
                       uint64_t* nsites) {
  MG_REQUIRE_READY();
  if (!h || !unpiled || !nsites || (h->nacc && (!alignments || !callable_sites || !polymorphic_sites || !pairs || !discordant)))
    return fail(MG_ERR_ARG, "null argument");
  if (min_depth < 2 || min_count < 1 || freq_permille > 500)
    return fail(MG_ERR_ARG, "min_depth %u (at least 2), min_count %u (at least 1), freq_permille %u (at most 500)", min_depth, min_count,
                freq_permille);
  hipStream_t st = ctx().stream;
  const uint64_t nacc = h->nacc;
  unsigned long long* sums = h->sums.as<unsigned long long>();
  unsigned long long* blk = h->blk.as<unsigned long long>();
  h->sites.release();
  h->npoly = 0;
  h->finished = false;
  if (nacc) MG_HIP(hipMemsetAsync(sums + nacc, 0, 4 * nacc * sizeof(uint64_t), st));
  if (h->nblocks) {
    const unsigned grid = var_grid(h->nblocks, kBlock / 64);
    {
      ProfScope ps("var_sums");
      hipLaunchKernelGGL(k_var_sites<false>, dim3(grid), dim3(kBlock), 0, st, h->cnt, h->nsites, h->nblocks, h->off.as<uint64_t>(), h->nacc,
                         sums, min_depth, min_count, freq_permille, sums + nacc, sums + 2 * nacc, sums + 3 * nacc, sums + 4 * nacc,
                         blk + 1, (mg_variant_site*)nullptr, (uint64_t)0);
      MG_HIP(hipGetLastError());
    }
    {
      ProfScope ps("var_scan");
      hipLaunchKernelGGL(k_var_scan, dim3(1), dim3(kScanBlock), 0, st, blk + 1, h->nblocks, blk);
      MG_HIP(hipGetLastError());
    }
    MG_HIP(hipMemcpyAsync(&h->npoly, blk, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
    if (h->npoly) {
      ProfScope ps("var_emit");
      MG_TRY(h->sites.alloc(h->npoly * sizeof(mg_variant_site)));
      hipLaunchKernelGGL(k_var_sites<true>, dim3(grid), dim3(kBlock), 0, st, h->cnt, h->nsites, h->nblocks, h->off.as<uint64_t>(), h->nacc,
                         sums, min_depth, min_count, freq_permille, sums + nacc, sums + 2 * nacc, sums + 3 * nacc, sums + 4 * nacc,
                         blk + 1, h->sites.as<mg_variant_site>(), h->npoly);
      MG_HIP(hipGetLastError());
    }
  }
  uint64_t* const out[5] = {alignments, callable_sites, polymorphic_sites, pairs, discordant};
  MG_TRY(fetch_sums(sums, nacc, out, 5, unpiled));
  *nsites = h->npoly;
  h->finished = true;
  return MG_OK;
}

int mg_variants_fetch_sites(mg_variants* h, mg_variant_site* out) {
  MG_REQUIRE_READY();
  if (!h) return fail(MG_ERR_ARG, "null argument");
  if (!h->finished) return fail(MG_ERR_STATE, "the sites are fetched after mg_variants_finish");
  if (h->npoly && !out) return fail(MG_ERR_ARG, "null argument");
  if (h->npoly) {
    hipStream_t st = ctx().stream;
    MG_HIP(hipMemcpyAsync(out, h->sites.p, h->npoly * sizeof(mg_variant_site), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
  }
  return MG_OK;
}

int mg_variants_consensus(mg_variants* h, const uint32_t* rows, uint32_t nrows, uint32_t min_depth, uint32_t min_count,
                          uint32_t freq_permille, uint32_t iupac, uint32_t width, uint8_t* out, uint64_t out_bytes) {
  MG_REQUIRE_READY();
  if (!h || (nrows && !rows) || (out_bytes && !out)) return fail(MG_ERR_ARG, "null argument");
  if (min_depth < 2 || min_count < 1 || freq_permille > 500)
    return fail(MG_ERR_ARG, "min_depth %u (at least 2), min_count %u (at least 1), freq_permille %u (at most 500)", min_depth, min_count,
                freq_permille);
  if (width < 1 || width > 65535) return fail(MG_ERR_ARG, "width %u (1 to 65535)", width);
  if (iupac > 1) return fail(MG_ERR_ARG, "iupac %u (0 or 1)", iupac);
  std::vector<uint64_t> toff(nrows + 1ull, 0);
  for (uint32_t r = 0; r < nrows; ++r) {
    if (rows[r] >= h->nacc) return fail(MG_ERR_ARG, "row %u: accession row %u (below %u)", r, rows[r], h->nacc);
    toff[r + 1] = toff[r] + mgvar::text_bytes(h->h_len[rows[r]], width);  // (a length is below 2^48: the check below keeps the sum in 64 bits)
    if (toff[r + 1] >> 62) return fail(MG_ERR_ARG, "rows 0 to %u: %llu bytes of text, too many for one call", r, (unsigned long long)toff[r + 1]);
  }
  const uint64_t total = toff[nrows];
  if (out_bytes != total)
    return fail(MG_ERR_ARG, "out_bytes %llu: the texts of these rows are %llu bytes", (unsigned long long)out_bytes, (unsigned long long)total);
  if (total == 0) return MG_OK;
  hipStream_t st = ctx().stream;
  DevBuf text, meta;  // u8[total rounded up to a word]; the offsets u64[nrows + 1], then the rows u32[nrows]
  const uint64_t off_bytes = (nrows + 1ull) * sizeof(uint64_t);
  if (text.alloc((total + 3) / 4 * 4) != MG_OK)
    return fail(MG_ERR_NOMEM, "the consensus text (%llu bytes) does not fit on the device: ask for fewer rows", (unsigned long long)total);
  MG_TRY(meta.alloc(off_bytes + (uint64_t)nrows * sizeof(uint32_t)));
  uint32_t* d_rows = reinterpret_cast<uint32_t*>(meta.as<uint8_t>() + off_bytes);
  MG_HIP(hipMemcpyAsync(meta.p, toff.data(), off_bytes, hipMemcpyHostToDevice, st));
  MG_HIP(hipMemcpyAsync(d_rows, rows, (uint64_t)nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const uint64_t nsteps = (total + kTextStep - 1) / kTextStep;
  {
    ProfScope ps("var_consensus");
    hipLaunchKernelGGL(k_var_consensus, dim3(var_grid(nsteps, kBlock / 64)), dim3(kBlock), 0, st, h->cnt, h->off.as<uint64_t>(),
                       h->len.as<uint64_t>(), meta.as<uint64_t>(), d_rows, nrows, total, nsteps, min_depth, min_count, freq_permille, iupac,
                       width, text.as<uint32_t>());
    MG_HIP(hipGetLastError());
  }
  MG_HIP(hipMemcpyAsync(out, text.p, total, hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));  // (toff and the caller's rows are free from here)
  return MG_OK;
}

int mg_variants_diff(mg_variants* h, const mg_refseq* ref, uint32_t min_depth, uint32_t min_count, uint32_t freq_permille,
                     uint64_t* compared, uint64_t* con_subs, uint64_t* pop_subs, uint64_t* ref_other, uint64_t* nsites) {
  MG_REQUIRE_READY();
  if (!h || !ref || !nsites || (h->nacc && (!compared || !con_subs || !pop_subs || !ref_other))) return fail(MG_ERR_ARG, "null argument");
  if (min_depth < 2 || min_count < 1 || freq_permille > 500)
    return fail(MG_ERR_ARG, "min_depth %u (at least 2), min_count %u (at least 1), freq_permille %u (at most 500)", min_depth, min_count,
                freq_permille);
  if (ref->nacc != h->nacc) return fail(MG_ERR_ARG, "the reference was parsed for %u accessions, the counts hold %u", ref->nacc, h->nacc);
  for (uint32_t a = 0; a < h->nacc; ++a)
    if (ref->h_len[a] != h->h_len[a])
      return fail(MG_ERR_ARG, "accession %u: the reference was parsed for length %llu, the counts hold %llu", a,
                  (unsigned long long)ref->h_len[a], (unsigned long long)h->h_len[a]);
  hipStream_t st = ctx().stream;
  const uint64_t nacc = h->nacc;
  h->dsites.release();
  h->ndiff = 0;
  h->diffed = false;
  MG_TRY(h->dsums.alloc((4 * nacc + 1) * sizeof(uint64_t)));
  MG_TRY(h->dblk.alloc((h->nblocks + 1) * sizeof(uint64_t)));
  unsigned long long* ds = h->dsums.as<unsigned long long>();
  unsigned long long* blk = h->dblk.as<unsigned long long>();
  const unsigned long long* aln = h->sums.as<unsigned long long>();
  MG_HIP(hipMemsetAsync(ds, 0, (4 * nacc + 1) * sizeof(uint64_t), st));
  if (h->nblocks) {
    const unsigned grid = var_grid(h->nblocks, kBlock / 64);
    {
      ProfScope ps("var_diff_sums");
      hipLaunchKernelGGL(k_var_diff<false>, dim3(grid), dim3(kBlock), 0, st, h->cnt, h->nsites, h->nblocks, h->off.as<uint64_t>(), h->nacc,
                         aln, ref->codes, ref->loaded.as<uint8_t>(), min_depth, min_count, freq_permille, ds, ds + nacc, ds + 2 * nacc,
                         ds + 3 * nacc, blk + 1, (mg_variant_diff*)nullptr, (uint64_t)0);
      MG_HIP(hipGetLastError());
    }
    {
      ProfScope ps("var_diff_scan");
      hipLaunchKernelGGL(k_var_scan, dim3(1), dim3(kScanBlock), 0, st, blk + 1, h->nblocks, blk);
      MG_HIP(hipGetLastError());
    }
    MG_HIP(hipMemcpyAsync(&h->ndiff, blk, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
    if (h->ndiff) {
      ProfScope ps("var_diff_emit");
      MG_TRY(h->dsites.alloc(h->ndiff * sizeof(mg_variant_diff)));
      hipLaunchKernelGGL(k_var_diff<true>, dim3(grid), dim3(kBlock), 0, st, h->cnt, h->nsites, h->nblocks, h->off.as<uint64_t>(), h->nacc,
                         aln, ref->codes, ref->loaded.as<uint8_t>(), min_depth, min_count, freq_permille, ds, ds + nacc, ds + 2 * nacc,
                         ds + 3 * nacc, blk + 1, h->dsites.as<mg_variant_diff>(), h->ndiff);
      MG_HIP(hipGetLastError());
    }
  }
  uint64_t* const out[4] = {compared, con_subs, pop_subs, ref_other};
  uint64_t none = 0;
  MG_TRY(fetch_sums(ds, nacc, out, 4, &none));
  *nsites = h->ndiff;
  h->diffed = true;
  return MG_OK;
}

int mg_variants_fetch_diffs(mg_variants* h, mg_variant_diff* out) {
  MG_REQUIRE_READY();
  if (!h) return fail(MG_ERR_ARG, "null argument");
  if (!h->diffed) return fail(MG_ERR_STATE, "the differing sites are fetched after mg_variants_diff");
  if (h->ndiff && !out) return fail(MG_ERR_ARG, "null argument");
  if (h->ndiff) {
    hipStream_t st = ctx().stream;
    MG_HIP(hipMemcpyAsync(out, h->dsites.p, h->ndiff * sizeof(mg_variant_diff), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
  }
  return MG_OK;
}

void mg_variants_free(mg_variants* h) { delete h; }

}  // extern "C"
