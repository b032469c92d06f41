// mg_depth.hip — per-base depth of coverage per accession (--depth, --depth_windows; metalign_amd/depth.py is the definition).
//
// One int32 slot per reference base plus one per accession, at 64-bit offsets (mg_depth_core.h).  Five kernels:
//
//   k_depth_add         records + places -> +1 at the first slot of every counting, placed record's clipped interval, -1 at the slot
//                       behind its last; the accession's alignments and the unplaced counted in hashed LDS bins (mg_side_dev.h: AccBins).
//                       The -1 lands inside the accession's own slots, so every accession's slots sum to zero.
//   k_depth_tile_sums   the sum of every kTile slots (64-bit), one wavefront per tile; a tile in which no accession with an alignment
//                       owns a slot is all zero and is not read (by this pass or by k_depth_hist).
//   k_depth_scan_tiles  the exclusive scan of the tile sums in place, by ONE workgroup walking them 4096 at a time
//                       (mg_side_dev.h: block_scan_excl).
//   k_depth_hist        reads the slots a second time: tile carry + scan within the tile = depth[p], never written back.  Every
//                       workgroup takes chunks of 64 tiles, four tiles behind one barrier, keeps a 4096-bin LDS histogram of the accession it is in and
//                       flushes the non-empty bins into that accession's row (64-bit adds) when the accession changes and at the
//                       end.  Accessions without a placed alignment have no row and are skipped (the host gives them {0: L}).
//                       Windows: depth_sum and covered of the windows a tile's part of an accession touches are summed in LDS and
//                       added once per window.
//   k_depth_win_compact the windows with depth_sum > 0 -> (accession, index, depth_sum, covered), one atomic per wavefront for the
//                       place; the host sorts them.
#include <algorithm>

#include "mg_internal.h"
#include "mg_depth_core.h"
#include "mg_side_dev.h"

using namespace mg;

struct mg_depth {
  int32_t* slots = nullptr;  // i32[ntiles * kTile] (its own allocation, as the coverage bitmap); zero behind nslots
  uint64_t nslots = 0, ntiles = 0, nwin = 0, nrows = 0, nnz = 0;
  uint32_t nacc = 0, window = 0;
  bool finished = false, rows_fetched = false, windows_fetched = false;
  DevBuf off;     // u64[nacc + 1]: accession a's first slot
  DevBuf sums;    // u64[nacc + 1]: alignments, unplaced
  DevBuf woff;    // u64[nacc + 1]: accession a's first window
  DevBuf wsum;    // u64[nwin]
  DevBuf wcov;    // u32[nwin]
  DevBuf carry;   // i64[ntiles]
  DevBuf rowmap;  // i32[nacc]: the histogram row of an accession, -1 without one
  DevBuf rows;    // u64[nrows * kDepthBins]
  DevBuf wout;    // mg_depth_window[nnz]
  DevBuf cursor;  // u64
  std::vector<uint32_t> row_acc;
  ~mg_depth() { if (slots) (void)hipFree(slots); }
};

namespace {

constexpr unsigned kBlock = 256, kBins = 1024, kScanBlock = 1024, kScanPer = 4;
constexpr unsigned kHistBatch = 4;
constexpr uint64_t kHistChunk = 64;  // tiles (a multiple of kHistBatch)
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr uint64_t kFlushTiles = 1ull << 21;  // an LDS bin counts at most 2^21 tiles of 2^10 slots

struct OffView {
  const uint64_t* p;
  __device__ uint64_t operator[](uint32_t i) const { return p[i]; }
};
struct RowView {
  const int32_t* p;
  __device__ int32_t operator[](uint32_t i) const { return p[i]; }
};

__global__ __launch_bounds__(kBlock) void k_depth_add(const mg_aln_rec* __restrict__ recs, const mg_aln_place* __restrict__ place,
                                                      uint64_t n, double pct_id, const uint64_t* __restrict__ off, uint32_t nacc,
                                                      int32_t* __restrict__ slots, unsigned long long* __restrict__ aln,
                                                      unsigned long long* __restrict__ unplaced) {
  __shared__ AccBins<kBins, 1, kBlock> bins;
  unsigned long long* const sums[1] = {aln};
  bins.init();
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    uint32_t a = 0;
    bool placed = false, unp = false;
    if (i < n) {
      const mg_aln_rec r = recs[i];
      if (mgv::counts(r, pct_id)) {
        const mg_aln_place pl = place[i];
        a = r.ref_new & MG_REC_REF_MASK;
        uint64_t o = 0, clen = 0;
        if (a < nacc) {
          o = off[a];
          clen = mgv::clipped(pl.pos0, pl.span, off[a + 1] - o - 1);
        }
        if (clen) {
          uint64_t plus, minus;
          mgd::diff_slots(o, pl.pos0, clen, &plus, &minus);  // (minus <= o + L: the accession's extra slot at the most)
          atomicAdd(&slots[plus], 1);
          atomicAdd(&slots[minus], -1);
          placed = true;
        } else {
          unp = true;
        }
      }
    }
    bins.count_one(unp);
    bins.add(placed, a, nullptr, sums);
  }
  bins.flush(sums, unplaced);
}

__global__ __launch_bounds__(kBlock) void k_depth_tile_sums(const int32_t* __restrict__ slots, uint64_t nslots, uint64_t ntiles,
                                                            const uint64_t* __restrict__ off, uint32_t nacc,
                                                            const int32_t* __restrict__ rowmap, long long* __restrict__ tsum) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const uint64_t nwaves = (uint64_t)gridDim.x * (kBlock / 64);
  // every wavefront takes a contiguous run of tiles and walks the accessions along with it
  const uint64_t per = (ntiles + nwaves - 1) / nwaves;
  const uint64_t t_beg = wave * per, t_end = t_beg + per < ntiles ? t_beg + per : ntiles;
  if (t_beg >= t_end) return;
  uint32_t a = mgv::owner_of(OffView{off}, nacc, t_beg * mgd::kTile);
  for (uint64_t t = t_beg; t < t_end; ++t) {
    const uint64_t s0 = t * mgd::kTile, s_end = s0 + mgd::kTile < nslots ? s0 + mgd::kTile : nslots;
    while (off[a + 1] <= s0) ++a;
    if (!mgd::tile_has_row(OffView{off}, RowView{rowmap}, nacc, a, s_end)) {  // (nothing was added here)
      if (lane == 0) tsum[t] = 0;
      continue;
    }
    const int4* p = reinterpret_cast<const int4*>(slots + s0);
    long long s = 0;
    for (unsigned k = 0; k < mgd::kTile / 256; ++k) {
      const int4 v = p[k * 64 + lane];
      s += (long long)v.x + v.y + v.z + v.w;
    }
    s = (long long)wave_sum((unsigned long long)s);
    if (lane == 0) tsum[t] = s;
  }
}

__global__ __launch_bounds__(kScanBlock) void k_depth_scan_tiles(long long* __restrict__ t, uint64_t n) {
  (void)block_scan_excl<long long, kScanBlock, kScanPer>(t, n, 0ll);
}

__global__ __launch_bounds__(kBlock) void k_depth_hist(const int32_t* __restrict__ slots, uint64_t nslots, uint64_t ntiles,
                                                       const long long* __restrict__ carry, const uint64_t* __restrict__ off,
                                                       uint32_t nacc, const int32_t* __restrict__ rowmap,
                                                       unsigned long long* __restrict__ rows, uint32_t W,
                                                       const uint64_t* __restrict__ woff, unsigned long long* __restrict__ wsum,
                                                       uint32_t* __restrict__ wcov) {
  __shared__ uint32_t s_hist[mgd::kDepthBins];
  __shared__ unsigned long long s_ws[mgd::kTile];
  __shared__ uint32_t s_wc[mgd::kTile];
  __shared__ long long s_wave[2][kHistBatch][kBlock / 64];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  for (unsigned i = tid; i < mgd::kDepthBins; i += kBlock) s_hist[i] = 0;
  for (unsigned i = tid; i < mgd::kTile; i += kBlock) { s_ws[i] = 0; s_wc[i] = 0; }
  __syncthreads();
  uint32_t hist_acc = kEmpty;  // the accession whose positions s_hist holds
  uint64_t since = 0;
  unsigned buf = 0;
  auto flush = [&](uint32_t acc) {
    __syncthreads();
    unsigned long long* row = rows + (uint64_t)rowmap[acc] * mgd::kDepthBins;
    for (unsigned b = tid; b < mgd::kDepthBins; b += kBlock) {
      const uint32_t c = s_hist[b];
      if (c) {
        atomicAdd(&row[b], (unsigned long long)c);
        s_hist[b] = 0;
      }
    }
    __syncthreads();
  };
  // One tile whose depths this thread holds in d4 (slots s0 + 4 tid ..); a = the accession of slot s0.  Uniform over the workgroup.
  auto tile = [&](uint64_t s0, uint32_t a, const uint32_t (&d4)[4]) {
    const uint64_t my = s0 + 4ull * tid;
    const uint64_t s_end = s0 + mgd::kTile < nslots ? s0 + mgd::kTile : nslots;
    uint64_t s = s0;
    while (s < s_end) {  // (the part of the tile that lies in one accession)
      while (off[a + 1] <= s) ++a;  // (s < nslots = off[nacc]: a stays below nacc)
      const uint64_t o = off[a], next = off[a + 1], L = next - o - 1;
      const uint64_t seg_e = next < s_end ? next : s_end;
      if (rowmap[a] >= 0) {
        if (hist_acc != a || since >= kFlushTiles) {
          if (hist_acc != kEmpty) flush(hist_acc);
          hist_acc = a;
          since = 0;
        }
        bool ok[4];
        uint32_t c4[4];
        for (unsigned k = 0; k < 4; ++k) {
          const uint64_t sk = my + k;
          ok[k] = sk >= s && sk < seg_e && mgd::is_base(sk, o, L);
          c4[k] = mgd::clamp(d4[k]);
        }
        // the histogram: one add per wavefront where it sees one depth, else one per run of a thread's slots
        const bool one = ok[0] && ok[1] && ok[2] && ok[3] && c4[0] == c4[1] && c4[1] == c4[2] && c4[2] == c4[3];
        const uint32_t c_first = __shfl(c4[0], 0, 64);
        if (__ballot(!(one && c4[0] == c_first)) == 0) {
          if (lane == 0) atomicAdd(&s_hist[c_first], 256u);
        } else {
          uint32_t run_c = 0, run_n = 0;
          for (unsigned k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            if (run_n && c4[k] != run_c) {
              atomicAdd(&s_hist[run_c], run_n);
              run_n = 0;
            }
            run_c = c4[k];
            ++run_n;
          }
          if (run_n) atomicAdd(&s_hist[run_c], run_n);
        }
        // the windows this part touches: at most kTile of them, summed in LDS, one global add each
        if (W && s - o < L) {
          const uint64_t end_p = seg_e - o < L ? seg_e - o : L;  // (positions [s - o, end_p))
          const uint64_t j_lo = mgd::window_of(s - o, W);
          const uint64_t nw = mgd::window_of(end_p - 1, W) - j_lo + 1;  // (<= kTile: at most kTile positions)
          bool act = false;
          uint64_t tj = 0, j = 0, r = 0;
          unsigned long long tsum = 0, tcov = 0;
          for (unsigned k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            if (!act) {
              j = mgd::window_of(my + k - o, W);
              r = (my + k - o) - j * W;
              act = true;
              tj = j;
            } else if (++r == W) {  // (a thread's valid slots are consecutive)
              r = 0;
              ++j;
            }
            if (j == tj) {
              tsum += d4[k];
              tcov += d4[k] != 0;
            } else if (d4[k]) {
              atomicAdd(&s_ws[j - j_lo], (unsigned long long)d4[k]);
              atomicAdd(&s_wc[j - j_lo], 1u);
            }
          }
          const unsigned long long am = __ballot(act);
          if (am) {
            const unsigned first = (unsigned)__builtin_ctzll(am);
            const unsigned long long jf = __shfl((unsigned long long)tj, (int)first, 64);
            if (__ballot(act && tj != jf) == 0) {
              const unsigned long long ws = wave_sum(act ? tsum : 0ull), wc = wave_sum(act ? tcov : 0ull);
              if (lane == first && ws) {
                atomicAdd(&s_ws[jf - j_lo], ws);
                atomicAdd(&s_wc[jf - j_lo], (uint32_t)wc);
              }
            } else if (act && tsum) {
              atomicAdd(&s_ws[tj - j_lo], tsum);
              atomicAdd(&s_wc[tj - j_lo], (uint32_t)tcov);
            }
          }
          __syncthreads();
          const uint64_t g0 = woff[a] + j_lo;  // (j_lo + nw - 1 = the window of a position below L: inside a's windows)
          for (uint64_t k = tid; k < nw; k += kBlock) {
            const unsigned long long ws = s_ws[k];
            if (ws) {
              atomicAdd(&wsum[g0 + k], ws);
              atomicAdd(&wcov[g0 + k], s_wc[k]);
              s_ws[k] = 0;
              s_wc[k] = 0;
            }
          }
          __syncthreads();
        }
      }
      s = seg_e;
    }
    ++since;
  };
  // Chunks of kHistChunk tiles go round the workgroups (a sample hits few accessions: a contiguous share per workgroup would leave
  // most of them idle); within a chunk kHistBatch tiles are loaded and scanned together, behind ONE barrier, and then taken one by one.
  const uint64_t nchunks = (ntiles + kHistChunk - 1) / kHistChunk;
  for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const uint64_t t1 = (chunk + 1) * kHistChunk < ntiles ? (chunk + 1) * kHistChunk : ntiles;
    uint32_t a = mgv::owner_of(OffView{off}, nacc, chunk * kHistChunk * mgd::kTile);  // (the chunk's first slot is below nslots)
    for (uint64_t tb = chunk * kHistChunk; tb < t1; tb += kHistBatch) {
      bool hit[kHistBatch];
      uint32_t a_of[kHistBatch];
      int4 v[kHistBatch];
      long long cy[kHistBatch];
      bool any = false;
#pragma unroll
      for (unsigned q = 0; q < kHistBatch; ++q) {
        hit[q] = false;
        a_of[q] = a;
        v[q] = make_int4(0, 0, 0, 0);
        cy[q] = 0;
        const uint64_t t = tb + q;
        if (t < t1) {
          const uint64_t s0 = t * mgd::kTile, s_end = s0 + mgd::kTile < nslots ? s0 + mgd::kTile : nslots;
          while (off[a + 1] <= s0) ++a;
          a_of[q] = a;
          hit[q] = mgd::tile_has_row(OffView{off}, RowView{rowmap}, nacc, a, s_end);  // (else every depth here is 0 and no row takes it)
          if (hit[q]) {
            v[q] = reinterpret_cast<const int4*>(slots + s0)[tid];  // (the slots are padded to whole tiles)
            cy[q] = carry[t];
            any = true;
          }
        }
      }
      if (!any) continue;  // (uniform)
      buf ^= 1u;  // (two buffers: the barrier of the next batch read lies between this one's reads and the writes of the one after)
      int x[kHistBatch][4];
      long long incl[kHistBatch];
#pragma unroll
      for (unsigned q = 0; q < kHistBatch; ++q) {
        x[q][0] = v[q].x;
        x[q][1] = x[q][0] + v[q].y;
        x[q][2] = x[q][1] + v[q].z;
        x[q][3] = x[q][2] + v[q].w;
        incl[q] = x[q][3];
        for (int d = 1; d < 64; d <<= 1) {
          const long long up = __shfl_up(incl[q], d, 64);
          if (lane >= (unsigned)d) incl[q] += up;
        }
        if (lane == 63) s_wave[buf][q][wv] = incl[q];
      }
      __syncthreads();
#pragma unroll
      for (unsigned q = 0; q < kHistBatch; ++q) {
        if (!hit[q]) continue;  // (uniform)
        long long base = cy[q] + incl[q] - x[q][3];
        for (unsigned w = 0; w < wv; ++w) base += s_wave[buf][q][w];
        const uint32_t d4[4] = {(uint32_t)(base + x[q][0]), (uint32_t)(base + x[q][1]), (uint32_t)(base + x[q][2]),
                                (uint32_t)(base + x[q][3])};
        tile((tb + q) * mgd::kTile, a_of[q], d4);
      }
    }
  }
  if (hist_acc != kEmpty) flush(hist_acc);
}

__global__ __launch_bounds__(kBlock) void k_depth_win_compact(const unsigned long long* __restrict__ wsum,
                                                              const uint32_t* __restrict__ wcov, uint64_t nwin,
                                                              const uint64_t* __restrict__ woff, uint32_t nacc,
                                                              mg_depth_window* __restrict__ out, uint64_t cap,
                                                              unsigned long long* __restrict__ cursor) {
  const unsigned lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < nwin; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t g = base + threadIdx.x;
    const unsigned long long ws = g < nwin ? wsum[g] : 0ull;
    const unsigned long long m = __ballot(ws != 0);
    if (!m) continue;
    const unsigned first = (unsigned)__builtin_ctzll(m);
    unsigned long long at = 0;
    if (lane == first) at = atomicAdd(cursor, (unsigned long long)__builtin_popcountll(m));
    at = __shfl(at, (int)first, 64);
    if (ws && out) {
      const uint64_t r = at + (uint64_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (r < cap) {
        const uint32_t a = mgv::owner_of(OffView{woff}, nacc, g);
        mg_depth_window w;
        w.index = g - woff[a];
        w.depth_sum = ws;
        w.acc = a;
        w.covered = wcov[g];
        out[r] = w;
      }
    }
  }
}

unsigned depth_grid(uint64_t items, unsigned per_block) { return side_grid(items, per_block, "depth_grid"); }

}  // namespace

extern "C" {

int mg_depth_create(const uint64_t* lengths, uint32_t nacc, uint32_t window, mg_depth** out) {
  MG_REQUIRE_READY();
  if (!out || (nacc && !lengths) || nacc > MG_REC_REF_MASK) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  hipStream_t st = ctx().stream;
  std::unique_ptr<mg_depth> d(new mg_depth());
  d->nacc = nacc;
  d->window = window;
  std::vector<uint64_t> h_off(nacc + 1ull, 0), h_woff(nacc + 1ull, 0);
  for (uint32_t a = 0; a < nacc; ++a) {
    if (lengths[a] >> 48) return fail(MG_ERR_ARG, "accession %u: length %llu", a, (unsigned long long)lengths[a]);
    h_off[a + 1] = h_off[a] + mgd::slots_of(lengths[a]);
    h_woff[a + 1] = h_woff[a] + mgd::windows_of_length(lengths[a], window);
  }
  d->nslots = h_off[nacc];
  d->ntiles = mgd::tiles_of(d->nslots);
  d->nwin = h_woff[nacc];
  MG_TRY(d->off.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(d->woff.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(d->sums.alloc((nacc + 1ull) * sizeof(uint64_t)));
  MG_TRY(d->rowmap.alloc((nacc + 1ull) * sizeof(int32_t)));
  MG_TRY(d->cursor.alloc(sizeof(uint64_t)));
  MG_TRY(d->carry.alloc((d->ntiles + 1) * sizeof(long long)));
  MG_TRY(d->wsum.alloc((d->nwin + 1) * sizeof(uint64_t)));
  MG_TRY(d->wcov.alloc((d->nwin + 1) * sizeof(uint32_t)));
  const uint64_t slot_bytes = d->ntiles * mgd::kTile * sizeof(int32_t) + 16;
  MG_TRY(own_alloc((void**)&d->slots, slot_bytes, "the depth slots (%llu bytes, four per reference base) do not fit: %s", slot_bytes));
  MG_HIP(hipMemsetAsync(d->slots, 0, slot_bytes, st));
  MG_HIP(hipMemsetAsync(d->sums.p, 0, (nacc + 1ull) * sizeof(uint64_t), st));
  MG_HIP(hipMemsetAsync(d->wsum.p, 0, (d->nwin + 1) * sizeof(uint64_t), st));
  MG_HIP(hipMemsetAsync(d->wcov.p, 0, (d->nwin + 1) * sizeof(uint32_t), st));
  MG_HIP(hipMemcpyAsync(d->off.p, h_off.data(), (nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipMemcpyAsync(d->woff.p, h_woff.data(), (nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipStreamSynchronize(st));  // (h_off and h_woff are free from here)
  *out = d.release();
  return MG_OK;
}

int mg_depth_add_dev(mg_depth* d, const mg_aln_rec* d_recs, const mg_aln_place* d_place, uint64_t n, double pct_id) {
  MG_REQUIRE_READY();
  if (!d || (n && (!d_recs || !d_place))) return fail(MG_ERR_ARG, "null argument");
  if (d->finished) return fail(MG_ERR_STATE, "mg_depth_add_dev after mg_depth_finish");
  if (n == 0) return MG_OK;
  ProfScope ps("depth_add");
  unsigned long long* sums = d->sums.as<unsigned long long>();
  hipLaunchKernelGGL(k_depth_add, dim3(depth_grid(n, kBlock)), dim3(kBlock), 0, ctx().stream, d_recs, d_place, n, pct_id,
                     d->off.as<uint64_t>(), d->nacc, d->slots, sums, sums + d->nacc);
  MG_HIP(hipGetLastError());
  return MG_OK;
}

int mg_depth_finish(mg_depth* d, uint64_t* alignments, uint64_t* unplaced, uint64_t* nrows, uint64_t* nwindows) {
  MG_REQUIRE_READY();
  if (!d || !unplaced || !nrows || !nwindows || (d->nacc && !alignments)) return fail(MG_ERR_ARG, "null argument");
  if (d->finished) return fail(MG_ERR_STATE, "mg_depth_finish called twice");
  hipStream_t st = ctx().stream;
  const uint64_t nacc = d->nacc;
  // the alignments first: only accessions that have one get a histogram row
  MG_TRY(fetch_sums(d->sums.p, nacc, &alignments, 1, unplaced));
  std::vector<int32_t> h_map(nacc + 1, -1);
  d->row_acc.clear();
  for (uint64_t a = 0; a < nacc; ++a) {
    if (alignments[a]) {
      h_map[a] = (int32_t)d->row_acc.size();
      d->row_acc.push_back((uint32_t)a);
    }
  }
  d->nrows = d->row_acc.size();
  MG_TRY(d->rows.alloc((d->nrows * mgd::kDepthBins + 1) * sizeof(uint64_t)));
  MG_HIP(hipMemsetAsync(d->rows.p, 0, (d->nrows * mgd::kDepthBins + 1) * sizeof(uint64_t), st));
  MG_HIP(hipMemcpyAsync(d->rowmap.p, h_map.data(), (nacc + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (d->nrows) {  // (without a placed alignment every depth is 0: nothing to scan)
    {
      ProfScope ps("depth_tile_sums");
      hipLaunchKernelGGL(k_depth_tile_sums, dim3(depth_grid(d->ntiles, kBlock / 64)), dim3(kBlock), 0, st, d->slots, d->nslots,
                         d->ntiles, d->off.as<uint64_t>(), d->nacc, d->rowmap.as<int32_t>(), d->carry.as<long long>());
      MG_HIP(hipGetLastError());
    }
    {
      ProfScope ps("depth_scan_tiles");
      hipLaunchKernelGGL(k_depth_scan_tiles, dim3(1), dim3(kScanBlock), 0, st, d->carry.as<long long>(), d->ntiles);
      MG_HIP(hipGetLastError());
    }
    {
      ProfScope ps("depth_hist");
      hipLaunchKernelGGL(k_depth_hist, dim3(depth_grid((d->ntiles + kHistChunk - 1) / kHistChunk, 1)), dim3(kBlock), 0, st, d->slots, d->nslots, d->ntiles,
                         d->carry.as<long long>(), d->off.as<uint64_t>(), d->nacc, d->rowmap.as<int32_t>(),
                         d->rows.as<unsigned long long>(), d->window, d->woff.as<uint64_t>(), d->wsum.as<unsigned long long>(),
                         d->wcov.as<uint32_t>());
      MG_HIP(hipGetLastError());
    }
  }
  d->nnz = 0;
  if (d->nrows && d->nwin) {
    ProfScope ps("depth_windows");
    unsigned long long* cur = d->cursor.as<unsigned long long>();
    const unsigned grid = depth_grid(d->nwin, kBlock);
    MG_HIP(hipMemsetAsync(cur, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_depth_win_compact, dim3(grid), dim3(kBlock), 0, st, d->wsum.as<unsigned long long>(), d->wcov.as<uint32_t>(),
                       d->nwin, d->woff.as<uint64_t>(), d->nacc, (mg_depth_window*)nullptr, (uint64_t)0, cur);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(&d->nnz, cur, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
    if (d->nnz) {
      MG_TRY(d->wout.alloc(d->nnz * sizeof(mg_depth_window)));
      MG_HIP(hipMemsetAsync(cur, 0, sizeof(uint64_t), st));
      hipLaunchKernelGGL(k_depth_win_compact, dim3(grid), dim3(kBlock), 0, st, d->wsum.as<unsigned long long>(),
                         d->wcov.as<uint32_t>(), d->nwin, d->woff.as<uint64_t>(), d->nacc, d->wout.as<mg_depth_window>(), d->nnz, cur);
      MG_HIP(hipGetLastError());
    }
  }
  MG_HIP(hipStreamSynchronize(st));
  // the slots and the dense windows have given what they hold
  (void)hipFree(d->slots);
  d->slots = nullptr;
  d->carry.release();
  d->wsum.release();
  d->wcov.release();
  d->finished = true;
  *nrows = d->nrows;
  *nwindows = d->nnz;
  return MG_OK;
}

int mg_depth_fetch_rows(mg_depth* d, uint32_t* accessions, uint64_t* hist) {
  MG_REQUIRE_READY();
  if (!d) return fail(MG_ERR_ARG, "null argument");
  if (!d->finished || d->rows_fetched) return fail(MG_ERR_STATE, "the histogram rows are fetched once, after mg_depth_finish");
  if (d->nrows && (!accessions || !hist)) return fail(MG_ERR_ARG, "null argument");
  hipStream_t st = ctx().stream;
  if (d->nrows) {
    MG_HIP(hipMemcpyAsync(hist, d->rows.p, d->nrows * mgd::kDepthBins * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
    std::copy(d->row_acc.begin(), d->row_acc.end(), accessions);
  }
  d->rows.release();
  d->rows_fetched = true;
  return MG_OK;
}

int mg_depth_fetch_windows(mg_depth* d, mg_depth_window* windows) {
  MG_REQUIRE_READY();
  if (!d) return fail(MG_ERR_ARG, "null argument");
  if (!d->finished || d->windows_fetched) return fail(MG_ERR_STATE, "the windows are fetched once, after mg_depth_finish");
  if (d->nnz && !windows) return fail(MG_ERR_ARG, "null argument");
  hipStream_t st = ctx().stream;
  if (d->nnz) {
    MG_HIP(hipMemcpyAsync(windows, d->wout.p, d->nnz * sizeof(mg_depth_window), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));
    std::sort(windows, windows + d->nnz, [](const mg_depth_window& x, const mg_depth_window& y) {
      return x.acc != y.acc ? x.acc < y.acc : x.index < y.index;
    });
  }
  d->wout.release();
  d->windows_fetched = true;
  return MG_OK;
}

void mg_depth_free(mg_depth* d) { delete d; }

}  // extern "C"
