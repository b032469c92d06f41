// mg_align.hip — short reads aligned to the reference codes by seed and extend (--aligner device; metalign_amd/align.py is the
// definition, mg_align_core.h holds the per-position rules, shared with the host check).  Reads (mg_reads) and reference
// (mg_refseq) are in HBM already; what comes out is an mg_sam_batch, as the tokenisers leave one.  No SAM text exists.
//
//   the index (mg_align_index_build)
//     k_al_ref<false>   one thread per reference base: is its k-mer position a minimizer (mga::minimizer_at)?  Counts them.
//     k_al_ref<true>    ... and writes (key, value), value = (pad(a) + p) << 1 | strand bit, through a cursor a wave moves once
//     sort_pairs_u64    by key; rle_keys + a scan: the unique keys with their runs' starts and lengths
//   a batch of reads (mg_align_reads_dev; the host halves a batch whose candidates do not fit)
//     k_al_seed<false>  one thread per read base: a minimizer?  Its key's run in the unique-key table; counts the entries
//     k_al_seed<true>   ... and writes one 64-bit candidate per entry: read << 40 | strand << 39 | (pad(a) + d)
//     sort_keys + rle   the DISTINCT candidates
//     k_al_extend       THE HOT PATH: one lane per distinct candidate scans its diagonal eight columns per step
//     compaction (k_al_compact): the accepted alignments
//     band > 0 (--align_band; mg_align_gap_core.h holds the per-cell rules):
//       k_al_gap_mark<false / true>   the REFINED ones (segment shorter than the read): counted with their workspace, then listed
//       k_al_gap        one wavefront per refined candidate: the banded table with affine gaps row by row, lane = band offset,
//                       four remembered bits per cell in LDS, then the walk back, which leaves the alignment's columns in HBM
//     pairs (--align_pairs interleaved; mg_align_pair_core.h holds the rules), between the extension and the compaction:
//       k_al_rescue_mark<false / true>   one thread per mate: its first R accepted candidates are anchors; counts, then lists, the
//                       windows in which the partner has no accepted candidate yet (the rescue tasks)
//       k_al_rescue     one wavefront per task: the partner read and the window of the reference in LDS, one diagonal per lane;
//                       the best diagonal as a candidate like a seeded one; sort + rle make them distinct, k_al_extend scans them
//                       and k_al_compact puts them behind the seeded
//     two stable sorts: the accepted alignments by (read, score descending, a, pos0, strand, d)
//     k_al_select<false / true>   one thread per read walks its list (overlap and secondary rules), counts, then writes records,
//                       places, edits, base entries and the pool
//     k_al_select_pair<false / true>   under pairs in its place: one thread per pair, the two lists in LDS, the pair choice
//
// pad(a) = off[a] + (a + 1) * 1024 keeps the diagonals of neighbouring accessions apart: d reaches from -(L - k) >= -1009 up to
// len[a] - 1, so pad(a) + d names (a, d) uniquely and a read never aligns across a boundary.  Everything is integers.
#include <memory>
#include <optional>
#include <vector>

#include "mg_align_core.h"
#include "mg_align_gap_core.h"
#include "mg_align_pair_core.h"
#include "mg_internal.h"

using namespace mg;

struct mg_align_index {
  uint32_t k = 0, w = 0, nacc = 0;
  uint64_t nsites = 0, nent = 0, nuniq = 0;
  DevBuf off;           // u64[nacc + 1]: the site offsets of the rows
  DevBuf keys, vals;    // u64[nent] each, by key
  DevBuf ukey, ustart;  // u64[nuniq] / u64[nuniq + 1]
  DevBuf ucount;        // u32[nuniq]
};

namespace {

constexpr int kAB = 256;
constexpr uint64_t kPad = 1024;
constexpr unsigned kReadShift = 40, kStrandShift = 39;
constexpr uint64_t kDiagMask = (1ull << kStrandShift) - 1;
constexpr uint64_t kMaxBatchReads = 1ull << 24;

struct Accepted {  // one accepted alignment: [b, e) of the oriented read on [pos0, pos0 + span) of row a
  uint32_t read, a, pos0;
  uint16_t score, b, e, span, nm, matched;  // nm: the edits; matched: the M columns
  uint16_t nops, strand;                    // nops: the columns of a refined alignment (0: ungapped, span M columns)
  uint64_t ops;                             // a refined one's columns in the workspace, the LAST column first
};

// the first sort's key: (a, pos0), then strand, then d ascending.  pos0 - d is b without gaps and within the band of it with them.
constexpr uint32_t kDiagOrder = 1023u + mga::kMaxBand;
__device__ __forceinline__ uint64_t key1_of(uint64_t site, uint32_t strand, int64_t pos0_minus_d) {
  return (site << 12) | ((uint64_t)strand << 11) | (uint64_t)((int64_t)kDiagOrder - pos0_minus_d);
}

__device__ __forceinline__ uint64_t pad_of(const uint64_t* __restrict__ off, uint64_t a) { return off[a] + (a + 1) * kPad; }

// the largest s in [lo, hi) with offs[s] <= g (offs[lo] <= g is the caller's)
__device__ __forceinline__ uint64_t seq_of(const uint64_t* __restrict__ offs, uint64_t lo, uint64_t hi, uint64_t g) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (offs[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Every lane of the wave: reserves `mine` slots behind *cursor, one atomic per wave; -> this lane's first slot.
__device__ __forceinline__ uint64_t wave_reserve(uint32_t mine, unsigned long long* cursor) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t x = mine;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  const uint32_t total = __shfl(x, 63, 64);
  unsigned long long base = 0;
  if (lane == 63 && total) base = atomicAdd(cursor, (unsigned long long)total);
  const uint32_t blo = __shfl((uint32_t)base, 63, 64), bhi = __shfl((uint32_t)(base >> 32), 63, 64);
  return (((uint64_t)bhi << 32) | blo) + (x - mine);
}

struct CodesAt {  // the reference: one code per byte
  const uint8_t* p;
  __device__ uint32_t operator()(uint64_t i) const { return p[i]; }
};
struct BasesAt {  // a read: the bytes as written
  const uint8_t* p;
  __device__ uint32_t operator()(uint64_t i) const { return mga::code_of(p[i]); }
};

template <bool kEmit>
__global__ __launch_bounds__(kAB) void k_al_ref(const uint8_t* __restrict__ codes, const uint64_t* __restrict__ off,
                                                const uint8_t* __restrict__ loaded, uint64_t nacc, uint64_t nsites, uint32_t k, uint32_t w,
                                                unsigned long long* __restrict__ cursor, uint64_t* __restrict__ keys,
                                                uint64_t* __restrict__ vals) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x; g0 < nsites; g0 += stride) {  // (uniform trips: the wave reserves together)
    const uint64_t g = g0 + threadIdx.x;
    bool is_min = false;
    mga::Key key{0, 0, false};
    uint64_t a = 0, p = 0;
    if (g < nsites) {
      a = seq_of(off, 0, nacc, g);
      const uint64_t n = off[a + 1] - off[a];
      p = g - off[a];
      if (loaded[a] && n >= k && p < n - k + 1) is_min = mga::minimizer_at(CodesAt{codes + off[a]}, n, p, k, w, &key);
    }
    const uint64_t at = wave_reserve(is_min ? 1u : 0u, cursor);
    if (kEmit && is_min) {
      keys[at] = key.key;
      vals[at] = ((pad_of(off, a) + p) << 1) | key.strand;
    }
  }
}

// the run of `key` in the unique-key table, or nuniq
__device__ __forceinline__ uint64_t find_key(const uint64_t* __restrict__ ukey, uint64_t nuniq, uint64_t key) {
  uint64_t lo = 0, hi = nuniq;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (ukey[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < nuniq && ukey[lo] == key ? lo : nuniq;
}

// reads [r0, r1), whose bases are [g_lo, g_hi) of `bases`
template <bool kEmit>
__global__ __launch_bounds__(kAB) void k_al_seed(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs, uint64_t r0,
                                                 uint64_t r1, uint64_t g_lo, uint64_t g_hi, uint32_t k, uint32_t w, uint32_t max_occ,
                                                 const uint64_t* __restrict__ ukey, const uint64_t* __restrict__ ustart,
                                                 const uint32_t* __restrict__ ucount, uint64_t nuniq, const uint64_t* __restrict__ vals,
                                                 unsigned long long* __restrict__ cursor, uint64_t* __restrict__ cand) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t g0 = g_lo + (uint64_t)blockIdx.x * blockDim.x; g0 < g_hi; g0 += stride) {
    const uint64_t g = g0 + threadIdx.x;
    uint32_t occ = 0, L = 0, i = 0;
    uint64_t r = 0, run = 0;
    mga::Key key{0, 0, false};
    if (g < g_hi) {
      r = seq_of(offs, r0, r1, g);
      const uint64_t n = offs[r + 1] - offs[r], p = g - offs[r];
      if (n >= k && n <= mga::kMaxRead && p < n - k + 1 && mga::minimizer_at(BasesAt{bases + offs[r]}, n, p, k, w, &key)) {
        const uint64_t u = find_key(ukey, nuniq, key.key);
        if (u < nuniq && ucount[u] <= max_occ) {
          occ = ucount[u];
          run = ustart[u];
          L = (uint32_t)n;
          i = (uint32_t)p;
        }
      }
    }
    const uint64_t at = wave_reserve(occ, cursor);
    if (kEmit) {
      for (uint32_t t = 0; t < occ; ++t) {
        const uint64_t v = vals[run + t];
        const uint64_t strand = (v & 1ull) ^ key.strand;
        const uint64_t shift = strand ? L - k - i : i;
        cand[at + t] = ((r - r0) << kReadShift) | (strand << kStrandShift) | ((v >> 1) - shift);
      }
    }
  }
}

// n <= 8 bytes at p, any alignment, from aligned 8-byte words: every word loaded holds one of the bytes
__device__ __forceinline__ uint64_t ld_bytes(const uint8_t* p, uint32_t n) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 7u);
  const uint64_t* a = reinterpret_cast<const uint64_t*>(p - sh);
  uint64_t v = a[0] >> (8u * sh);
  if (sh + n > 8u) v |= a[1] << (64u - 8u * sh);
  return v;
}

// the row of pad(a) + d: the largest a with off[a] + a * 1024 <= G
__device__ __forceinline__ uint64_t row_of(const uint64_t* __restrict__ off, uint64_t nacc, uint64_t G) {
  uint64_t lo = 0, hi = nacc;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] + mid * kPad <= G) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One lane per distinct candidate.  The columns outside the accession only reset the scan, and none of them lies between two inside
// columns, so the scan runs over the inside columns [j_lo, j_hi) alone, starting there.  Eight columns per step: the reference codes
// and the read's bytes each come as one 64-bit value (the read's reversed for strand 1).
__global__ __launch_bounds__(kAB) void k_al_extend(const uint64_t* __restrict__ cand, uint64_t ncand, uint64_t r0,
                                                   const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs,
                                                   const uint8_t* __restrict__ codes, const uint64_t* __restrict__ off, uint64_t nacc,
                                                   int32_t P, uint32_t min_score, uint2* __restrict__ ext, uint32_t* __restrict__ flag) {
  uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; c < ncand; c += stride) {
    const uint64_t cv = cand[c];
    const uint64_t r = r0 + (cv >> kReadShift), G = cv & kDiagMask;
    const bool rev = (cv >> kStrandShift) & 1ull;
    const uint64_t a = row_of(off, nacc, G);
    const int64_t d = (int64_t)G - (int64_t)pad_of(off, a);
    const int64_t len = (int64_t)(off[a + 1] - off[a]);
    const uint8_t* read = bases + offs[r];
    const int32_t L = (int32_t)(offs[r + 1] - offs[r]);
    const uint8_t* ref = codes + off[a];
    const int32_t j_lo = d < 0 ? (int32_t)-d : 0;
    const int32_t j_hi = len - d < (int64_t)L ? (int32_t)(len - d) : L;
    mga::Scan s;
    s.start = j_lo;
    for (int32_t j = j_lo; j < j_hi; j += 8) {
      const uint32_t n = j_hi - j < 8 ? (uint32_t)(j_hi - j) : 8u;
      uint64_t gw = ld_bytes(ref + (d + j), n), rw;
      if (rev) rw = __builtin_bswap64(ld_bytes(read + (L - j - (int32_t)n), n) << (8u * (8u - n)));
      else rw = ld_bytes(read + j, n);
#pragma unroll
      for (uint32_t t = 0; t < 8; ++t) {
        if (t < n) {
          uint32_t rc = mga::code_of((uint32_t)(rw >> (8u * t)) & 0xffu);
          if (rev) rc = mga::comp(rc);
          mga::step(s, j + (int32_t)t, true, rc < 4 && rc == ((uint32_t)(gw >> (8u * t)) & 0xffu), P);
        }
      }
    }
    ext[c] = make_uint2((uint32_t)s.best, ((uint32_t)s.b << 16) | (uint32_t)s.e);
    flag[c] = (uint32_t)s.best >= min_score ? 1u : 0u;
  }
}

// the accepted candidates, compacted behind the `base` there are already (the rescued ones go behind the seeded): their
// alignments, the first sort's keys (key1_of) and their own indices as the values
__global__ __launch_bounds__(kAB) void k_al_compact(const uint64_t* __restrict__ cand, const uint2* __restrict__ ext,
                                                    const uint32_t* __restrict__ flag, const uint64_t* __restrict__ at, uint64_t ncand,
                                                    const uint64_t* __restrict__ off, uint64_t nacc, uint32_t P, uint64_t base,
                                                    Accepted* __restrict__ acc, uint64_t* __restrict__ key1,
                                                    uint64_t* __restrict__ val) {
  uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; c < ncand; c += stride) {
    if (!flag[c]) continue;
    const uint64_t cv = cand[c], G = cv & kDiagMask, o = base + at[c];
    const uint64_t a = row_of(off, nacc, G);
    const int64_t d = (int64_t)G - (int64_t)pad_of(off, a);
    const uint2 x = ext[c];
    Accepted al;
    al.read = (uint32_t)(cv >> kReadShift);
    al.a = (uint32_t)a;
    al.b = (uint16_t)(x.y >> 16);
    al.e = (uint16_t)(x.y & 0xffffu);
    al.pos0 = (uint32_t)(d + al.b);
    al.score = (uint16_t)x.x;
    al.span = al.matched = (uint16_t)(al.e - al.b);
    al.nm = (uint16_t)mga::nm_of(al.span, x.x, P);
    al.nops = 0;
    al.strand = (uint16_t)((cv >> kStrandShift) & 1ull);
    al.ops = 0;
    acc[o] = al;
    key1[o] = key1_of(off[a] + al.pos0, al.strand, al.b);
    val[o] = o;
  }
}

// the most columns a refined alignment of an L-base read takes: M + I <= L, and D <= 2B + I (the band)
__device__ __forceinline__ uint32_t gap_ops_cap(uint32_t L, uint32_t B) { return 2u * L + 2u * B; }

// The refined candidates among the accepted: the segment is shorter than the read.  kEmit = false counts them (cur[0]), their
// workspace bytes (cur[1]) and their longest read (cur[2]); kEmit = true lists them and gives each its place in the workspace.
template <bool kEmit>
__global__ __launch_bounds__(kAB) void k_al_gap_mark(Accepted* __restrict__ acc, uint64_t n, uint64_t r0,
                                                     const uint64_t* __restrict__ offs, uint32_t B,
                                                     unsigned long long* __restrict__ cur, uint32_t* __restrict__ list) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t o0 = (uint64_t)blockIdx.x * blockDim.x; o0 < n; o0 += stride) {  // (uniform trips: the wave reserves together)
    const uint64_t o = o0 + threadIdx.x;
    uint32_t cap = 0, L = 0;
    if (o < n) {
      const uint64_t r = r0 + acc[o].read;
      L = (uint32_t)(offs[r + 1] - offs[r]);
      if ((uint32_t)acc[o].e - acc[o].b < L) cap = gap_ops_cap(L, B);
    }
    const uint64_t at = wave_reserve(cap ? 1u : 0u, cur), at_ops = wave_reserve(cap, cur + 1);
    if (!cap) continue;
    if (kEmit) {
      list[at] = (uint32_t)o;
      acc[o].ops = at_ops;
    } else {
      atomicMax(cur + 2, (unsigned long long)L);
    }
  }
}

constexpr uint32_t kNoCell = 0xffu;  // in the staged window of the reference: a column outside the accession

// what a wavefront of k_al_gap keeps in LDS for reads of up to max_len bases: the remembered bits (eight rows of a lane in one
// word), the oriented read's codes, and the window [d - B, d + L + B) of the reference
__host__ __device__ inline uint32_t gap_tb_words(uint32_t max_len) { return (max_len + 7u) / 8u * 64u; }
__host__ __device__ inline uint32_t gap_read_bytes(uint32_t max_len) { return (max_len + 3u) & ~3u; }
__host__ __device__ inline uint32_t gap_lds_bytes(uint32_t max_len, uint32_t B) {
  return gap_tb_words(max_len) * 4u + gap_read_bytes(max_len) + ((max_len + 2u * B + 3u) & ~3u);
}

// One wavefront per refined candidate, lane t = the band offset j - i - d + B, one read row per step.  X takes the lane's own H of the
// row before, I the H and I of lane t + 1's (one move down the lanes), D the largest offer of the lanes below in this row (an
// exclusive prefix maximum: log2 of the band steps up the lanes).  Each cell's four bits go to LDS, eight rows of a lane per
// word; the walk back reads them, every lane alike, and lane 0 writes the columns.  Strand 1 is reversed and complemented while
// the read is staged.  Nothing outside [0, n) of the candidate's accession is read: the window is staged under that test.
__global__ __launch_bounds__(64) void k_al_gap(const uint32_t* __restrict__ list, uint64_t nref, uint64_t r0,
                                               const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs,
                                               const uint8_t* __restrict__ codes, const uint64_t* __restrict__ off, int32_t P, int32_t B,
                                               int32_t O, int32_t E, uint32_t max_len, Accepted* __restrict__ acc,
                                               uint64_t* __restrict__ key1, uint8_t* __restrict__ ops) {
  extern __shared__ uint32_t gap_lds[];
  uint32_t* tb = gap_lds;
  uint8_t* rd = reinterpret_cast<uint8_t*>(gap_lds + gap_tb_words(max_len));
  uint8_t* gw = rd + gap_read_bytes(max_len);
  const int32_t t = (int32_t)threadIdx.x;
  const bool in_band = t <= 2 * B;
  for (uint64_t x = blockIdx.x; x < nref; x += gridDim.x) {
    const uint32_t o = list[x];
    const Accepted al = acc[o];
    const uint64_t r = r0 + al.read;
    const uint8_t* read = bases + offs[r];
    const int32_t L = (int32_t)(offs[r + 1] - offs[r]);
    const uint8_t* ref = codes + off[al.a];
    const int64_t n = (int64_t)(off[al.a + 1] - off[al.a]);
    const int64_t d = (int64_t)al.pos0 - (int64_t)al.b;
    __syncthreads();  // (the walk of the candidate before has read the LDS)
    if ((uint32_t)L <= max_len) {
      for (int32_t i = t; i < L; i += 64) {
        const uint32_t c = mga::code_of(read[al.strand ? L - 1 - i : i]);
        rd[i] = (uint8_t)(al.strand ? mga::comp(c) : c);
      }
      for (int32_t u = t; u < L + 2 * B; u += 64) {
        const int64_t j = d - B + u;
        gw[u] = j >= 0 && j < n ? ref[j] : (uint8_t)kNoCell;
      }
    }
    __syncthreads();
    if ((uint32_t)L > max_len) continue;  // (never: max_len is the longest refined read's)
    int32_t Hp = 0, Ip = mga::kGapNone;
    uint32_t best = 0, word = 0;
    for (int32_t i = 0; i < L; ++i) {
      const uint32_t oc = rd[i], gc = in_band ? gw[i + t] : kNoCell;
      const bool ex = gc != kNoCell;
      const int32_t h_up = __shfl_down(Hp, 1, 64), i_up = __shfl_down(Ip, 1, 64);
      const bool up_ex = ex && i > 0 && t < 2 * B;  // cell (i - 1, j): the same column, a row above, offset t + 1
      const int32_t X = Hp + mga::gap_sub(oc, gc, P);
      const int32_t I = mga::gap_ins(up_ex, h_up, i_up, O, E);
      const int32_t Hq = mga::gap_max(mga::gap_max(0, X), I);
      int32_t pm = __shfl_up(mga::gap_del_offer(ex, Hq, t, E), 1, 64);
      if (t == 0) pm = mga::kGapNone;
      for (int32_t s = 1; s <= 2 * B; s <<= 1) {
        const int32_t y = __shfl_up(pm, s, 64);
        if (t >= s) pm = mga::gap_max(pm, y);
      }
      const int32_t D = ex ? mga::gap_del_prefix(pm, t, O, E) : mga::kGapNone;
      const int32_t H = ex ? mga::gap_h(X, I, D) : 0;
      const int32_t h_left = __shfl_up(H, 1, 64);
      word |= mga::gap_bits(H, X, I, D, Hp, h_up, h_left, O, E) << (4u * ((uint32_t)i & 7u));
      if (((uint32_t)i & 7u) == 7u || i == L - 1) {
        tb[((uint32_t)i >> 3) * 64u + (uint32_t)t] = word;
        word = 0;
      }
      if (ex && H > 0) {
        const uint32_t key = mga::gap_best_pack(H, i, t);
        best = key > best ? key : best;
      }
      Hp = H;
      Ip = ex ? I : mga::kGapNone;
    }
#pragma unroll
    for (int32_t s = 32; s > 0; s >>= 1) {
      const uint32_t y = (uint32_t)__shfl_xor((int32_t)best, s, 64);
      best = y > best ? y : best;
    }
    __syncthreads();  // (the bits of every lane are in LDS)
    if (best == 0) continue;  // (never: the band holds the diagonal, whose scan was accepted)
    mga::GapWalk w;
    w.i = mga::gap_best_i(best);
    w.t = mga::gap_best_t(best);
    const int32_t e = w.i + 1;
    const int64_t j_end = w.i + d + w.t - B;
    const uint32_t cap = gap_ops_cap((uint32_t)L, (uint32_t)B);
    uint32_t nops = 0, nm = 0, matched = 0;
    uint8_t* out = ops + al.ops;
    while (!w.done && w.i >= 0 && w.t >= 0 && w.t <= 2 * B && nops < cap) {
      const int32_t ci = w.i, ct = w.t;
      const uint32_t nib = (uint32_t)__builtin_amdgcn_readfirstlane(
          (int32_t)((tb[((uint32_t)ci >> 3) * 64u + (uint32_t)ct] >> (4u * ((uint32_t)ci & 7u))) & 15u));
      const int32_t op = mga::gap_walk(w, nib);
      if (op < 0) continue;
      if (op == (int32_t)mga::kOpM) {
        ++matched;
        if (mga::gap_sub(rd[ci], gw[ci + ct], P) < 0) ++nm;
      } else {
        ++nm;
      }
      if (t == 0) out[nops] = (uint8_t)op;
      ++nops;
    }
    if (t == 0) {
      const int64_t pos0 = w.i + d + w.t - B;
      Accepted up = al;
      up.pos0 = (uint32_t)pos0;
      up.score = (uint16_t)mga::gap_best_h(best);
      up.b = (uint16_t)w.i;
      up.e = (uint16_t)e;
      up.span = (uint16_t)(j_end - pos0 + 1);
      up.nm = (uint16_t)nm;
      up.matched = (uint16_t)matched;
      up.nops = (uint16_t)nops;
      acc[o] = up;
      key1[o] = key1_of(off[al.a] + up.pos0, al.strand, pos0 - d);
    }
  }
}

// the second sort's keys, in the first sort's order: read << 11 | 1024 - score
__global__ __launch_bounds__(kAB) void k_al_key2(const Accepted* __restrict__ acc, const uint64_t* __restrict__ order, uint64_t n,
                                                 uint64_t* __restrict__ key2) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const Accepted al = acc[order[i]];
    key2[i] = ((uint64_t)al.read << 11) | (1024u - al.score);
  }
}

__device__ __forceinline__ uint64_t lower_bound(const uint64_t* __restrict__ v, uint64_t n, uint64_t x) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- pairs (--align_pairs interleaved; mg_align_pair_core.h holds the rules): reads 2i and 2i + 1 of a range are the mates of pair i

struct RescueTask {  // the partner read `read` sought on strand `strand` of row a over the diagonals lo .. lo + ndiag - 1
  uint32_t read, a;
  int64_t lo;
  uint32_t ndiag, strand;
};

// the key of order_key among the accepted candidates of ONE read before refinement: score descending, (a, pos0), strand, d
// (d = pos0 - b: ascending d is descending b)
__device__ __forceinline__ uint64_t anchor_key(uint32_t score, uint64_t site, uint32_t strand, uint32_t b) {
  return ((uint64_t)(1024u - score) << 51) | (site << 12) | ((uint64_t)strand << 11) | (uint64_t)(1023u - b);
}

// The accepted candidate of [i0, i1) with the smallest anchor_key above `prev` (any, when !have_prev) -> its index, or i1.
__device__ __forceinline__ uint64_t next_anchor(const uint64_t* __restrict__ dist, const uint2* __restrict__ ext,
                                                const uint32_t* __restrict__ flag, uint64_t i0, uint64_t i1,
                                                const uint64_t* __restrict__ off, uint64_t nacc, bool have_prev, uint64_t prev,
                                                uint64_t* key_out) {
  uint64_t at = i1, best = 0;
  for (uint64_t i = i0; i < i1; ++i) {
    if (!flag[i]) continue;
    const uint64_t cv = dist[i], G = cv & kDiagMask;
    const uint64_t a = row_of(off, nacc, G);
    const int64_t d = (int64_t)G - (int64_t)pad_of(off, a);
    const uint2 x = ext[i];
    const uint32_t b = x.y >> 16;
    const uint64_t key = anchor_key(x.x, off[a] + (uint64_t)(d + (int64_t)b), (uint32_t)((cv >> kStrandShift) & 1ull), b);
    if (have_prev && key <= prev) continue;
    if (at == i1 || key < best) {
      at = i;
      best = key;
    }
  }
  *key_out = best;
  return at;
}

// The task of the anchor at index i of read q's candidates, if it has one: the window is not empty and the partner's candidates
// hold no accepted one within the band of it.
__device__ __forceinline__ bool rescue_task_of(const uint64_t* __restrict__ dist, const uint32_t* __restrict__ flag, uint64_t ndist,
                                               uint64_t i, uint64_t q, uint32_t L, uint32_t Lp, const uint64_t* __restrict__ off,
                                               uint64_t nacc, uint32_t I, uint32_t B, RescueTask* task) {
  const uint64_t cv = dist[i], G = cv & kDiagMask;
  const uint64_t a = row_of(off, nacc, G), pad = pad_of(off, a);
  const int64_t d = (int64_t)G - (int64_t)pad, n = (int64_t)(off[a + 1] - off[a]);
  const uint32_t strand = (uint32_t)((cv >> kStrandShift) & 1ull), sp = 1u - strand;
  int64_t lo, hi;
  if (!mga::rescue_window(strand, d, L, Lp, n, I, &lo, &hi)) return false;
  // (a candidate of the partner has 1 - L' <= d'' <= n - 1: the band's ends beyond that hold none, and stay off the neighbours' diagonals)
  const int64_t dlo = lo - (int64_t)B < 1 - (int64_t)Lp ? 1 - (int64_t)Lp : lo - (int64_t)B;
  const int64_t dhi = hi + (int64_t)B > n - 1 ? n - 1 : hi + (int64_t)B;
  const uint64_t head = ((q ^ 1ull) << kReadShift) | ((uint64_t)sp << kStrandShift);
  const uint64_t k_lo = head | (uint64_t)((int64_t)pad + dlo), k_hi = head | (uint64_t)((int64_t)pad + dhi);
  for (uint64_t c = lower_bound(dist, ndist, k_lo); c < ndist && dist[c] <= k_hi; ++c)
    if (flag[c]) return false;
  task->read = (uint32_t)(q ^ 1ull);
  task->a = (uint32_t)a;
  task->lo = lo;
  task->ndiag = (uint32_t)(hi - lo + 1);
  task->strand = sp;
  return true;
}

// One thread per read (mate) of the range: its first R accepted candidates by order_key are its anchors; each may give a task.
// kEmit = false counts the tasks (cur[0]); kEmit = true writes them.  Both judge the candidates as the extension left them.
template <bool kEmit>
__global__ __launch_bounds__(kAB) void k_al_rescue_mark(const uint64_t* __restrict__ dist, const uint2* __restrict__ ext,
                                                        const uint32_t* __restrict__ flag, uint64_t ndist, uint64_t r0, uint64_t nreads,
                                                        const uint64_t* __restrict__ offs, const uint64_t* __restrict__ off, uint64_t nacc,
                                                        uint32_t k, uint32_t R, uint32_t I, uint32_t B,
                                                        unsigned long long* __restrict__ cur, RescueTask* __restrict__ tasks) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x; q0 < nreads; q0 += stride) {  // (uniform trips: the wave reserves together)
    const uint64_t q = q0 + threadIdx.x;
    uint64_t i0 = 0, i1 = 0;
    uint32_t L = 0, Lp = 0, mine = 0;
    if (q < nreads) {
      L = (uint32_t)(offs[r0 + q + 1] - offs[r0 + q]);
      Lp = (uint32_t)(offs[r0 + (q ^ 1ull) + 1] - offs[r0 + (q ^ 1ull)]);
      if (Lp >= k && Lp <= mga::kMaxRead) {
        i0 = lower_bound(dist, ndist, q << kReadShift);
        i1 = lower_bound(dist, ndist, (q + 1) << kReadShift);
      }
    }
    RescueTask task;
    for (uint32_t pass = 0; pass < (kEmit ? 2u : 1u); ++pass) {  // (emit: count, reserve, then write)
      uint64_t at = 0;
      if (kEmit && pass == 1) at = wave_reserve(mine, cur);
      uint64_t prev = 0;
      uint32_t n = 0;
      for (uint32_t r = 0; r < R && i0 < i1; ++r) {
        uint64_t key;
        const uint64_t i = next_anchor(dist, ext, flag, i0, i1, off, nacc, r > 0, prev, &key);
        if (i == i1) break;
        prev = key;
        if (!rescue_task_of(dist, flag, ndist, i, q, L, Lp, off, nacc, I, B, &task)) continue;
        if (kEmit && pass == 1) tasks[at + n] = task;
        ++n;
      }
      if (pass == 0) mine = n;
    }
    if (!kEmit) wave_reserve(mine, cur);
  }
}

// what a wavefront of k_al_rescue keeps in LDS: the oriented partner read's codes (1024 bytes) and the window of the reference,
// at most max_insert codes (the diagonals of a window and the read's columns span no more), with eight bytes the word loads may
// touch behind it
__host__ __device__ inline uint32_t rescue_win_bytes(uint32_t max_insert) { return ((max_insert + 3u) & ~3u) + 8u; }
__host__ __device__ inline uint32_t rescue_lds_bytes(uint32_t max_insert) { return mga::kMaxRead + rescue_win_bytes(max_insert); }

// One wavefront per task.  The oriented partner read and the reference window [lo, lo + ndiag + L' - 1) of the task's accession
// alone are staged in LDS once, columns outside [0, n) as no cell.  Lane t scans the diagonals lo + t, lo + t + 64, ..., four
// columns per step: the read's four codes are one word, the same for every lane, the window's four come from two aligned words.
// The wave reduces to (score, smallest d') and lane 0 writes the candidate in the seeds' 64-bit form, or ~0 below min_score.
__global__ __launch_bounds__(64) void k_al_rescue(const RescueTask* __restrict__ tasks, uint64_t ntasks, uint64_t r0,
                                                  const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs,
                                                  const uint8_t* __restrict__ codes, const uint64_t* __restrict__ off, int32_t P,
                                                  uint32_t min_score, uint32_t max_insert, uint64_t* __restrict__ out) {
  extern __shared__ uint32_t resc_lds[];
  uint8_t* rd = reinterpret_cast<uint8_t*>(resc_lds);
  uint8_t* gw = rd + mga::kMaxRead;
  const uint32_t* rd4 = resc_lds;
  const uint32_t* gw4 = resc_lds + mga::kMaxRead / 4u;
  const uint32_t t = threadIdx.x, win = rescue_win_bytes(max_insert) - 8u;
  for (uint64_t x = blockIdx.x; x < ntasks; x += gridDim.x) {
    const RescueTask task = tasks[x];
    const uint64_t r = r0 + task.read;
    const uint8_t* read = bases + offs[r];
    const uint32_t Lp = (uint32_t)(offs[r + 1] - offs[r]), W = task.ndiag;
    const uint8_t* ref = codes + off[task.a];
    const int64_t n = (int64_t)(off[task.a + 1] - off[task.a]);
    const bool fits = Lp >= 1 && Lp <= mga::kMaxRead && W >= 1 && (uint64_t)W + Lp - 1 <= win;
    __syncthreads();  // (the scans of the task before have read the LDS)
    if (fits) {
      for (uint32_t i = t; i < Lp; i += 64) {
        const uint32_t c = mga::code_of(read[task.strand ? Lp - 1 - i : i]);
        rd[i] = (uint8_t)(task.strand ? mga::comp(c) : c);
      }
      for (uint32_t u = t; u < W + Lp - 1; u += 64) {
        const int64_t j = task.lo + (int64_t)u;
        gw[u] = j >= 0 && j < n ? ref[j] : (uint8_t)kNoCell;
      }
    }
    __syncthreads();
    uint64_t best = 0;
    if (fits) {  // (never otherwise: the mark kernel's windows span at most max_insert codes)
      for (uint32_t w = t; w < W; w += 64) {
        mga::Scan s;
        for (uint32_t j = 0; j < Lp; j += 4) {
          const uint32_t at = w + j, lo4 = gw4[at >> 2], hi4 = gw4[(at >> 2) + 1];
          const uint32_t g4 = __builtin_amdgcn_alignbyte(hi4, lo4, at & 3u), r4 = rd4[j >> 2];
#pragma unroll
          for (uint32_t c = 0; c < 4; ++c) {
            if (j + c < Lp) {
              const uint32_t gc = (g4 >> (8u * c)) & 0xffu, rc = (r4 >> (8u * c)) & 0xffu;
              mga::step(s, (int32_t)(j + c), gc != kNoCell, rc < 4 && rc == gc, P);
            }
          }
        }
        const uint64_t key = ((uint64_t)(uint32_t)s.best << 32) | (uint64_t)(0xffffffffu - w);
        if (s.best > 0 && key > best) best = key;
      }
    }
#pragma unroll
    for (int32_t sh = 32; sh > 0; sh >>= 1) {
      const uint32_t ylo = (uint32_t)__shfl_xor((int32_t)(uint32_t)best, sh, 64);
      const uint32_t yhi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(best >> 32), sh, 64);
      const uint64_t y = ((uint64_t)yhi << 32) | ylo;
      best = y > best ? y : best;
    }
    if (t == 0) {
      uint64_t cand = ~0ull;
      if ((uint32_t)(best >> 32) >= min_score) {
        const int64_t d = task.lo + (int64_t)(0xffffffffu - (uint32_t)best);
        cand = ((uint64_t)task.read << kReadShift) | ((uint64_t)task.strand << kStrandShift) |
               (uint64_t)((int64_t)pad_of(off, task.a) + d);
      }
      out[x] = cand;
    }
  }
}

constexpr uint32_t kGapCode = 5;  // a reference base under a deletion, in the pile (mg_variants_core.h)

struct BatchOut {  // where the batch's arrays go on from: the records in front of this call's, the pool bytes likewise
  mg_aln_rec* recs;
  mg_aln_place* places;
  mg_aln_edit* edits;
  mg_aln_bases* bases;
  uint8_t* pool;
  uint64_t pool_base;
};

// One record at place o of this call's, with the side arrays the batch carries: an alignment of a read of L bases (`read`: its
// bytes).  A primary carries len(SEQ) and its codes, which go to the pool at pa.
__device__ __forceinline__ void write_record(const BatchOut& out, uint64_t o, const Accepted& al, uint32_t L, uint32_t flag, bool is_new,
                                             bool primary, uint64_t pa, const uint8_t* __restrict__ read, const uint8_t* __restrict__ ops) {
  const uint32_t span = al.span;
  mg_aln_rec rec;
  rec.ref_new = al.a | (is_new ? MG_REC_NEW_BIT : 0u);
  rec.matched = al.matched;
  rec.total = L + (span - al.matched);  // (every CIGAR operation, as the tokenisers count a line: L and the D columns)
  rec.flag_len = flag | ((primary ? L : 0u) << MG_REC_LEN_SHIFT);
  out.recs[o] = rec;
  if (out.places) out.places[o] = mg_aln_place{al.pos0, span};
  if (out.edits) out.edits[o] = mg_aln_edit{al.nm, al.nops ? al.nops : span};
  if (!out.bases) return;
  if (!primary) {
    out.bases[o] = mg_aln_bases{0, 0, 0};
    return;
  }
  out.bases[o] = mg_aln_bases{out.pool_base + pa, al.pos0, span};
  uint8_t* dst = out.pool + out.pool_base + pa;
  if (al.nops) {  // a refined alignment: M gives the read's code, D the gap's, I is skipped; span codes in all
    uint32_t col = al.b, j = 0, byte = 0;
    for (uint32_t c = al.nops; c-- > 0;) {
      const uint32_t op = ops[al.ops + c];
      if (op != mga::kOpI) {
        const uint32_t cd = op == mga::kOpD ? kGapCode
                            : al.strand     ? mga::comp(mga::code_of(read[L - 1 - col]))
                                            : mga::code_of(read[col]);
        byte |= cd << (4u * (j & 1u));
        if (j & 1u) {
          dst[j >> 1] = (uint8_t)byte;
          byte = 0;
        }
        ++j;
      }
      if (op != mga::kOpD) ++col;
    }
    if (j & 1u) dst[j >> 1] = (uint8_t)byte;
  } else {
    for (uint32_t j = 0; j < span; j += 2) {
      uint32_t byte = 0;
      for (uint32_t t = 0; t < 2 && j + t < span; ++t) {
        const uint32_t col = al.b + j + t;
        const uint32_t cd = al.strand ? mga::comp(mga::code_of(read[L - 1 - col])) : mga::code_of(read[col]);
        byte |= cd << (4u * t);
      }
      dst[j >> 1] = (uint8_t)byte;
    }
  }
}

// One thread per read of the batch walks its accepted alignments in order.  kEmit = false: nkept[r], npool[r] = the bytes its
// primary's codes take.  kEmit = true: the records and their side arrays at rec_at[r], the codes at pool_at[r].
template <bool kEmit>
__global__ __launch_bounds__(kAB) void k_al_select(const Accepted* __restrict__ acc, const uint64_t* __restrict__ key2,
                                                   const uint64_t* __restrict__ order, uint64_t nacc_aln, uint64_t r0, uint64_t nreads,
                                                   const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs,
                                                   const uint8_t* __restrict__ ops, uint32_t max_secondary, uint32_t sec_pct, uint32_t* __restrict__ nkept,
                                                   uint32_t* __restrict__ npool, unsigned long long* __restrict__ aligned,
                                                   const uint64_t* __restrict__ rec_at, const uint64_t* __restrict__ pool_at, BatchOut out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x; q0 < nreads; q0 += stride) {  // (uniform trips: the ballot)
    const uint64_t q = q0 + threadIdx.x;
    uint32_t kept = 0;
    if (q < nreads) {
      const uint64_t lo = lower_bound(key2, nacc_aln, q << 11), hi = lower_bound(key2, nacc_aln, (q + 1) << 11);
      const uint32_t L = (uint32_t)(offs[r0 + q + 1] - offs[r0 + q]);
      uint32_t ka[mga::kMaxSecondary + 1], ks[mga::kMaxSecondary + 1], kp[mga::kMaxSecondary + 1], ke[mga::kMaxSecondary + 1];
      uint32_t best = 0, pool_bytes = 0;
      for (uint64_t i = lo; i < hi && kept < 1 + max_secondary; ++i) {
        const Accepted al = acc[order[i]];
        const uint32_t span = al.span, end = al.pos0 + span;
        bool ok = kept == 0 || mga::secondary_ok(al.score, best, sec_pct);
        for (uint32_t t = 0; ok && t < kept; ++t) ok = !mga::overlaps(ka[t], ks[t], kp[t], ke[t], al.a, al.strand, al.pos0, end);
        if (!ok) continue;
        if (kept == 0) {
          best = al.score;
          pool_bytes = (span + 1) / 2;
        }
        if (kEmit)
          write_record(out, rec_at[q] + kept, al, L, 16u * al.strand + (kept ? 256u : 0u), kept == 0, kept == 0,
                       kept == 0 && out.bases ? pool_at[q] : 0, bases + offs[r0 + q], ops);
        ka[kept] = al.a;
        ks[kept] = al.strand;
        kp[kept] = al.pos0;
        ke[kept] = end;
        ++kept;
      }
      if (!kEmit) {
        nkept[q] = kept;
        npool[q] = pool_bytes;
      }
    }
    if (!kEmit) {
      const unsigned long long m = __ballot(kept != 0);
      if (m && (threadIdx.x & 63u) == 0) atomicAdd(aligned, (unsigned long long)__builtin_popcountll(m));
    }
  }
}

// The selection under pairs.  One THREAD per pair, its two lists C1 and C2 (sixteen entries each at the most) in LDS, five words per
// entry laid out [word][entry][thread], so that a wavefront's accesses fall on 64 consecutive words: 40 KiB per workgroup of one
// wavefront.  In registers the 2 x 16 x 5 words would spill; a wavefront per pair would leave 48 of its lanes idle on the usual
// lists of one or two entries.  The walk is the definition's: the lists under the overlap rule, the best concordant pair, the
// secondaries by their best concordant partner, or each mate alone.  kEmit as k_al_select's, per read (mate).
constexpr uint32_t kPairWords = 5;  // a, pos0, span | b << 16, e | score << 11 | strand << 22, the place among the sorted
constexpr int kPB = 64;

struct PairListAt {  // a mate's list as mg_align_pair_core.h reads it
  const uint32_t (*w)[2 * mga::kPairList][kPB];
  uint32_t first, tid, L;
  __device__ mga::PairAln operator()(uint32_t i) const {
    const uint32_t e = first + i, sb = w[2][e][tid], es = w[3][e][tid];
    return mga::pair_aln(w[0][e][tid], (es >> 22) & 1u, (es >> 11) & 0x7ffu, w[1][e][tid], sb & 0xffffu, sb >> 16, es & 0x7ffu, L);
  }
};

template <bool kEmit>
__global__ __launch_bounds__(kPB) void k_al_select_pair(const Accepted* __restrict__ acc, const uint64_t* __restrict__ key2,
                                                        const uint64_t* __restrict__ order, uint64_t nacc_aln, uint64_t r0, uint64_t nreads,
                                                        const uint8_t* __restrict__ bases, const uint64_t* __restrict__ offs,
                                                        const uint8_t* __restrict__ ops, uint32_t max_secondary, uint32_t sec_pct,
                                                        uint32_t max_insert, uint32_t* __restrict__ nkept, uint32_t* __restrict__ npool,
                                                        unsigned long long* __restrict__ aligned, unsigned long long* __restrict__ proper_pairs,
                                                        const uint64_t* __restrict__ rec_at, const uint64_t* __restrict__ pool_at, BatchOut out) {
  __shared__ uint32_t w[kPairWords][2 * mga::kPairList][kPB];
  const uint32_t tid = threadIdx.x;
  const uint64_t npairs = nreads / 2, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x; p0 < npairs; p0 += stride) {  // (uniform trips: the ballots)
    const uint64_t pr = p0 + tid;
    uint32_t kept[2] = {0, 0};
    bool proper = false;
    if (pr < npairs) {
      uint32_t cnt[2], L[2];
      for (uint32_t m = 0; m < 2; ++m) {
        const uint64_t q = 2 * pr + m;
        const uint64_t lo = lower_bound(key2, nacc_aln, q << 11), hi = lower_bound(key2, nacc_aln, (q + 1) << 11);
        L[m] = (uint32_t)(offs[r0 + q + 1] - offs[r0 + q]);
        uint32_t n = 0;
        for (uint64_t i = lo; i < hi && n < mga::kPairList; ++i) {
          const Accepted al = acc[order[i]];
          const uint32_t end = al.pos0 + al.span;
          bool ok = true;
          for (uint32_t t = 0; ok && t < n; ++t) {
            const uint32_t e = m * mga::kPairList + t, sb = w[2][e][tid];
            ok = !mga::overlaps(w[0][e][tid], (w[3][e][tid] >> 22) & 1u, w[1][e][tid], w[1][e][tid] + (sb & 0xffffu), al.a, al.strand,
                                al.pos0, end);
          }
          if (!ok) continue;
          const uint32_t e = m * mga::kPairList + n;
          w[0][e][tid] = al.a;
          w[1][e][tid] = al.pos0;
          w[2][e][tid] = (uint32_t)al.span | ((uint32_t)al.b << 16);
          w[3][e][tid] = (uint32_t)al.e | ((uint32_t)al.score << 11) | ((uint32_t)al.strand << 22);
          w[4][e][tid] = (uint32_t)(i - lo);
          ++n;
        }
        cnt[m] = n;
      }
      const PairListAt list[2] = {{w, 0, tid, L[0]}, {w, mga::kPairList, tid, L[1]}};
      uint32_t own[2] = {0, 0}, best = 0;
      proper = mga::pair_best(list[0], cnt[0], list[1], cnt[1], (int64_t)max_insert, &own[0], &own[1], &best);
      // which entries a mate keeps, in the order of its records: bit t of take[m], the primary apart
      uint32_t take[2] = {0, 0}, primary[2] = {0, 0};
      for (uint32_t m = 0; m < 2; ++m) {
        uint32_t n = 0;
        if (proper) {
          primary[m] = own[m];
          n = 1;
          for (uint32_t t = 0; t < cnt[m] && n < 1 + max_secondary; ++t) {
            if (t == own[m]) continue;
            const mga::PairAln x = list[m](t);
            uint32_t partner = 0;
            if (mga::pair_partner(x, list[1 - m], cnt[1 - m], (int64_t)max_insert, &partner) &&
                mga::pair_secondary_ok(x.score, partner, best, sec_pct)) {
              take[m] |= 1u << t;
              ++n;
            }
          }
        } else if (cnt[m]) {  // alone: the list is in order and free of overlaps; the share of the best score and the cut remain
          const uint32_t top = list[m](0).score;
          n = 1;
          for (uint32_t t = 1; t < cnt[m] && n < 1 + max_secondary; ++t) {
            if (mga::secondary_ok(list[m](t).score, top, sec_pct)) {
              take[m] |= 1u << t;
              ++n;
            }
          }
        }
        kept[m] = n;
      }
      if (kEmit) {
        for (uint32_t m = 0; m < 2; ++m) {
          if (!kept[m]) continue;
          const uint64_t q = 2 * pr + m, lo = lower_bound(key2, nacc_aln, q << 11);
          const bool partner_has = kept[1 - m] != 0;
          const uint32_t partner_strand = partner_has ? (w[3][(1 - m) * mga::kPairList + primary[1 - m]][tid] >> 22) & 1u : 0u;
          const uint8_t* read = bases + offs[r0 + q];
          uint32_t t_rec = 0;
          for (uint32_t pass = 0; pass < 2; ++pass) {  // the primary, then the secondaries in the list's order
            for (uint32_t t = 0; t < cnt[m]; ++t) {
              if (pass == 0 ? t != primary[m] : !((take[m] >> t) & 1u)) continue;
              const Accepted al = acc[order[lo + w[4][m * mga::kPairList + t][tid]]];
              const uint32_t flag = mga::pair_flag(m, t_rec, al.strand, partner_has, partner_strand, proper);
              write_record(out, rec_at[q] + t_rec, al, L[m], flag, t_rec == 0 && (m == 0 || kept[0] == 0), t_rec == 0,
                           t_rec == 0 && out.bases ? pool_at[q] : 0, read, ops);
              ++t_rec;
            }
          }
        }
      } else {
        for (uint32_t m = 0; m < 2; ++m) {
          nkept[2 * pr + m] = kept[m];
          npool[2 * pr + m] = kept[m] ? ((w[2][m * mga::kPairList + primary[m]][tid] & 0xffffu) + 1u) / 2u : 0u;
        }
      }
    }
    if (!kEmit) {
      const unsigned long long m0 = __ballot(kept[0] != 0), m1 = __ballot(kept[1] != 0), mp = __ballot(proper);
      if (tid == 0) {
        if (m0 | m1) atomicAdd(aligned, (unsigned long long)(__builtin_popcountll(m0) + __builtin_popcountll(m1)));
        if (mp) atomicAdd(proper_pairs, (unsigned long long)__builtin_popcountll(mp));
      }
    }
  }
}

unsigned al_grid(uint64_t items) { return grid_cap(grid_for(items, kAB, (unsigned)ctx().num_cus * 8), "align_grid"); }

int fetch_u64(const void* d, uint64_t* h) {
  hipStream_t st = ctx().stream;
  MG_HIP(hipMemcpyAsync(h, d, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));
  return MG_OK;
}

// what the library may still take: free memory and its own cached blocks
int mem_room(uint64_t* room) {
  uint64_t f = 0, t = 0, pooled = 0;
  MG_TRY(mg_mem_info(&f, &t, &pooled));
  *room = f + pooled;
  return MG_OK;
}

// A side array of the batch grown to hold `need` bytes, its first `have` bytes kept.
int grow(DevBuf& buf, uint64_t have, uint64_t need) {
  if (buf.p && buf.bytes >= need) return MG_OK;
  DevBuf nb;
  const uint64_t want = buf.p ? (need > 2 * buf.bytes ? need : 2 * buf.bytes) : need;
  if (nb.alloc(want < 256 ? 256 : want) != MG_OK) return MG_ERR_NOMEM;
  if (have) MG_HIP(hipMemcpyAsync(nb.p, buf.p, have, hipMemcpyDeviceToDevice, ctx().stream));
  MG_HIP(hipStreamSynchronize(ctx().stream));  // (the old block goes back to the pool behind the copy)
  buf = std::move(nb);
  return MG_OK;
}

struct AlignJob {
  const mg_align_index* ix;
  const mg_refseq* ref;
  const uint8_t* d_bases;
  const uint64_t* d_offs;
  mg_align_params p;
  mg_align_gap gap;
  mg_align_pairs pairs;
  unsigned want;
  mg_sam_batch* sb;
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [5] the refined candidates, [6] the rescued ones accepted, [7] the proper pairs
};

// a rescue task, its candidate, the sorted copy, the distinct one and its count, the scan result, flag and place
constexpr uint64_t kBytesPerTask = sizeof(RescueTask) + 8 + 8 + 8 + 4 + 8 + 4 + 8;
constexpr uint64_t kBytesPerCand = 64;  // the candidate, its sorted copy, the distinct one and its count, the radix sort's own, the scan result and flag, the scan's words

// reads [r0, r1) -> their records behind the batch's; halves the range while its candidates do not fit.  Under pairs r0 and r1 are
// even and so is every cut: a pair is never parted.
int align_range(AlignJob& j, uint64_t r0, uint64_t r1) {
  if (r1 - r0 > kMaxBatchReads) {
    for (uint64_t r = r0; r < r1; r += kMaxBatchReads) MG_TRY(align_range(j, r, r + kMaxBatchReads < r1 ? r + kMaxBatchReads : r1));
    return MG_OK;
  }
  Context& c = ctx();
  hipStream_t st = c.stream;
  const mg_align_index* ix = j.ix;
  const uint64_t nreads = r1 - r0;
  uint64_t g[2] = {0, 0};
  MG_TRY(fetch_u64(j.d_offs + r0, &g[0]));
  MG_TRY(fetch_u64(j.d_offs + r1, &g[1]));
  // [0] the cursor, [1] the distinct candidates, [2] the aligned reads, [3] the proper pairs, [4 .. 6] the refined: their number,
  // workspace bytes, longest read, [8] the rescue tasks, [9] their distinct candidates
  DevBuf small;
  MG_TRY(small.alloc(12 * sizeof(uint64_t)));
  unsigned long long* d_cursor = small.as<unsigned long long>();
  MG_HIP(hipMemsetAsync(small.p, 0, 12 * sizeof(uint64_t), st));
  const bool paired = j.pairs.interleaved != 0;
  const uint64_t unit = paired ? 2 : 1;
  const char* one = paired ? "pair" : "read";
  const uint64_t mid = r0 + nreads / 2 / unit * unit;  // (where a range that does not fit is cut)
  uint64_t ncand = 0;
  if (g[1] > g[0] && ix->nuniq) {
    ProfScope ps("align_seed");
    hipLaunchKernelGGL(k_al_seed<false>, dim3(al_grid(g[1] - g[0])), dim3(kAB), 0, st, j.d_bases, j.d_offs, r0, r1, g[0], g[1], j.p.k,
                       j.p.w, j.p.max_occ, ix->ukey.as<uint64_t>(), ix->ustart.as<uint64_t>(), ix->ucount.as<uint32_t>(), ix->nuniq,
                       ix->vals.as<uint64_t>(), d_cursor, (uint64_t*)nullptr);
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_u64(d_cursor, &ncand));
  }
  uint64_t room = 0;
  MG_TRY(mem_room(&room));
  uint64_t budget = room / 2 / kBytesPerCand;
  if (budget > 0xfffffff0ull) budget = 0xfffffff0ull;  // (the run-length encoder counts in 32 bits)
  if (dbg("align_batch_cands") > 0) budget = (uint64_t)dbg("align_batch_cands");
  if (ncand > budget) {
    if (nreads < 2 * unit)
      return fail(MG_ERR_NOMEM, "the %llu candidates of one %s (%llu bytes) do not fit on the device", (unsigned long long)ncand, one,
                  (unsigned long long)(ncand * kBytesPerCand));
    small.release();
    MG_TRY(align_range(j, r0, mid));
    return align_range(j, mid, r1);
  }
  j.stats[0] += nreads;
  mg_sam_batch* sb = j.sb;
  uint64_t ndist = 0, nacc_aln = 0;
  DevBuf cand, sorted, dist, counts, ext, flag, at, acc, k1, v1, k2, v2, gap_list, gap_ops;
  DevBuf tasks, rcand, rsorted, rdist, rcounts, rext, rflag, rat;  // the rescue's
  uint64_t nrd = 0, nresc = 0;
  if (ncand) {
    if (cand.alloc(ncand * 8) != MG_OK || sorted.alloc(ncand * 8) != MG_OK || dist.alloc(ncand * 8) != MG_OK ||
        counts.alloc(ncand * 4) != MG_OK)
      return fail(MG_ERR_NOMEM, "the %llu candidates of a batch (%llu bytes) do not fit on the device", (unsigned long long)ncand,
                  (unsigned long long)(ncand * kBytesPerCand));
    MG_HIP(hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st));
    {
      ProfScope ps("align_seed");
      hipLaunchKernelGGL(k_al_seed<true>, dim3(al_grid(g[1] - g[0])), dim3(kAB), 0, st, j.d_bases, j.d_offs, r0, r1, g[0], g[1], j.p.k,
                         j.p.w, j.p.max_occ, ix->ukey.as<uint64_t>(), ix->ustart.as<uint64_t>(), ix->ucount.as<uint32_t>(), ix->nuniq,
                         ix->vals.as<uint64_t>(), d_cursor, cand.as<uint64_t>());
      MG_HIP(hipGetLastError());
    }
    {
      ProfScope ps("align_unique");
      MG_TRY(sort_keys(cand.as<uint64_t>(), sorted.as<uint64_t>(), ncand, 64));
      MG_TRY(rle_keys(sorted.as<uint64_t>(), ncand, dist.as<uint64_t>(), counts.as<uint32_t>(), small.as<uint64_t>() + 1));
    }
    MG_TRY(fetch_u64(small.as<uint64_t>() + 1, &ndist));
    cand.release();
    sorted.release();
    counts.release();
  }
  if (ndist) {
    if (ext.alloc(ndist * sizeof(uint2)) != MG_OK || flag.alloc(ndist * 4) != MG_OK || at.alloc((ndist + 1) * 8) != MG_OK)
      return fail(MG_ERR_NOMEM, "the %llu distinct candidates of a batch do not fit on the device", (unsigned long long)ndist);
    {
      ProfScope ps("align_extend");
      hipLaunchKernelGGL(k_al_extend, dim3(al_grid(ndist)), dim3(kAB), 0, st, dist.as<uint64_t>(), ndist, r0, j.d_bases, j.d_offs,
                         j.ref->codes, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, (int32_t)j.p.mismatch, j.p.min_score, ext.as<uint2>(),
                         flag.as<uint32_t>());
      MG_HIP(hipGetLastError());
    }
    MG_TRY(exclusive_sum_u32_to_u64(flag.as<uint32_t>(), at.as<uint64_t>(), ndist, &nacc_aln));
  }
  const uint64_t nseeded = nacc_aln;
  if (paired && j.pairs.rescue && nseeded) {
    // mate rescue: the tasks are counted first, and their bytes join the arithmetic of a range that does not fit
    std::optional<ProfScope> pr;
    pr.emplace("align_rescue");
    uint64_t ntasks = 0;
    hipLaunchKernelGGL(k_al_rescue_mark<false>, dim3(al_grid(nreads)), dim3(kAB), 0, st, dist.as<uint64_t>(), ext.as<uint2>(),
                       flag.as<uint32_t>(), ndist, r0, nreads, j.d_offs, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, j.p.k, j.pairs.rescue,
                       j.pairs.max_insert, j.gap.band, d_cursor + 8, (RescueTask*)nullptr);
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_u64(d_cursor + 8, &ntasks));
    if (ntasks) {
      MG_TRY(mem_room(&room));
      uint64_t task_budget = room / 2;
      if (dbg("align_rescue_bytes") > 0) task_budget = (uint64_t)dbg("align_rescue_bytes");
      if (ntasks * kBytesPerTask > task_budget) {
        if (nreads < 2 * unit)
          return fail(MG_ERR_NOMEM, "the %llu rescue tasks of one pair (%llu bytes) do not fit on the device", (unsigned long long)ntasks,
                      (unsigned long long)(ntasks * kBytesPerTask));
        j.stats[0] -= nreads;
        pr.reset();  // (the halves' own families are theirs)
        for (DevBuf* b : {&small, &dist, &ext, &flag, &at}) b->release();
        MG_TRY(align_range(j, r0, mid));
        return align_range(j, mid, r1);
      }
      if (tasks.alloc(ntasks * sizeof(RescueTask)) != MG_OK || rcand.alloc(ntasks * 8) != MG_OK || rsorted.alloc(ntasks * 8) != MG_OK ||
          rdist.alloc(ntasks * 8) != MG_OK || rcounts.alloc(ntasks * 4) != MG_OK)
        return fail(MG_ERR_NOMEM, "the %llu rescue tasks of a batch (%llu bytes) do not fit on the device", (unsigned long long)ntasks,
                    (unsigned long long)(ntasks * kBytesPerTask));
      MG_HIP(hipMemsetAsync(d_cursor + 8, 0, sizeof(uint64_t), st));
      hipLaunchKernelGGL(k_al_rescue_mark<true>, dim3(al_grid(nreads)), dim3(kAB), 0, st, dist.as<uint64_t>(), ext.as<uint2>(),
                         flag.as<uint32_t>(), ndist, r0, nreads, j.d_offs, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, j.p.k, j.pairs.rescue,
                         j.pairs.max_insert, j.gap.band, d_cursor + 8, tasks.as<RescueTask>());
      MG_HIP(hipGetLastError());
      const unsigned grid = grid_cap(grid_for(ntasks, 1, (unsigned)c.num_cus * 32), "align_grid");
      hipLaunchKernelGGL(k_al_rescue, dim3(grid), dim3(64), rescue_lds_bytes(j.pairs.max_insert), st, tasks.as<RescueTask>(), ntasks, r0,
                         j.d_bases, j.d_offs, j.ref->codes, ix->off.as<uint64_t>(), (int32_t)j.p.mismatch, j.p.min_score, j.pairs.max_insert,
                         rcand.as<uint64_t>());
      MG_HIP(hipGetLastError());
      // two anchors that found one diagonal give it once; a task that found nothing gave ~0, the last of the sorted if there is one
      MG_TRY(sort_keys(rcand.as<uint64_t>(), rsorted.as<uint64_t>(), ntasks, 64));
      MG_TRY(rle_keys(rsorted.as<uint64_t>(), ntasks, rdist.as<uint64_t>(), rcounts.as<uint32_t>(), small.as<uint64_t>() + 9));
      MG_TRY(fetch_u64(small.as<uint64_t>() + 9, &nrd));
      uint64_t last = 0;
      if (nrd) MG_TRY(fetch_u64(rdist.as<uint64_t>() + (nrd - 1), &last));
      if (nrd && last == ~0ull) --nrd;
      for (DevBuf* b : {&tasks, &rcand, &rsorted, &rcounts}) b->release();
      if (nrd) {
        if (rext.alloc(nrd * sizeof(uint2)) != MG_OK || rflag.alloc(nrd * 4) != MG_OK || rat.alloc((nrd + 1) * 8) != MG_OK)
          return fail(MG_ERR_NOMEM, "the %llu rescued candidates of a batch do not fit on the device", (unsigned long long)nrd);
        // the rescued diagonals' segments, by the kernel that scans the seeded ones
        hipLaunchKernelGGL(k_al_extend, dim3(al_grid(nrd)), dim3(kAB), 0, st, rdist.as<uint64_t>(), nrd, r0, j.d_bases, j.d_offs,
                           j.ref->codes, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, (int32_t)j.p.mismatch, j.p.min_score, rext.as<uint2>(),
                           rflag.as<uint32_t>());
        MG_HIP(hipGetLastError());
        MG_TRY(exclusive_sum_u32_to_u64(rflag.as<uint32_t>(), rat.as<uint64_t>(), nrd, &nresc));
        nacc_aln += nresc;
      }
    }
  }
  std::optional<ProfScope> ps;  // (the selection's family; the refinement between its launches is a family of its own)
  ps.emplace("align_select");
  if (nacc_aln) {
    if (acc.alloc(nacc_aln * sizeof(Accepted)) != MG_OK || k1.alloc(nacc_aln * 8) != MG_OK || v1.alloc(nacc_aln * 8) != MG_OK ||
        k2.alloc(nacc_aln * 8) != MG_OK || v2.alloc(nacc_aln * 8) != MG_OK)
      return fail(MG_ERR_NOMEM, "the %llu accepted alignments of a batch do not fit on the device", (unsigned long long)nacc_aln);
    hipLaunchKernelGGL(k_al_compact, dim3(al_grid(ndist)), dim3(kAB), 0, st, dist.as<uint64_t>(), ext.as<uint2>(), flag.as<uint32_t>(),
                       at.as<uint64_t>(), ndist, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, j.p.mismatch, (uint64_t)0, acc.as<Accepted>(),
                       k1.as<uint64_t>(), v1.as<uint64_t>());
    MG_HIP(hipGetLastError());
    if (nresc) {  // the rescued, behind the seeded: from here on they are accepted alignments like any other
      hipLaunchKernelGGL(k_al_compact, dim3(al_grid(nrd)), dim3(kAB), 0, st, rdist.as<uint64_t>(), rext.as<uint2>(), rflag.as<uint32_t>(),
                         rat.as<uint64_t>(), nrd, ix->off.as<uint64_t>(), (uint64_t)ix->nacc, j.p.mismatch, nseeded, acc.as<Accepted>(),
                         k1.as<uint64_t>(), v1.as<uint64_t>());
      MG_HIP(hipGetLastError());
    }
    if (j.gap.band) {
      // the refined candidates: counted with their workspace first, which joins the arithmetic of a range that does not fit
      ps.reset();
      std::optional<ProfScope> pg;
      pg.emplace("align_refine");
      uint64_t g3[3] = {0, 0, 0};
      hipLaunchKernelGGL(k_al_gap_mark<false>, dim3(al_grid(nacc_aln)), dim3(kAB), 0, st, acc.as<Accepted>(), nacc_aln, r0, j.d_offs,
                         j.gap.band, d_cursor + 4, (uint32_t*)nullptr);
      MG_HIP(hipGetLastError());
      MG_HIP(hipMemcpyAsync(g3, d_cursor + 4, sizeof(g3), hipMemcpyDeviceToHost, st));
      MG_HIP(hipStreamSynchronize(st));
      const uint64_t nrefined = g3[0], ops_bytes = g3[1], need = nrefined * 4 + ops_bytes;
      if (nrefined) {
        MG_TRY(mem_room(&room));
        uint64_t ws_budget = room / 2;
        if (dbg("align_gap_bytes") > 0) ws_budget = (uint64_t)dbg("align_gap_bytes");
        if (need > ws_budget) {
          if (nreads < 2 * unit)
            return fail(MG_ERR_NOMEM, "the %llu refined candidates of one %s (%llu bytes) do not fit on the device",
                        (unsigned long long)nrefined, one, (unsigned long long)need);
          j.stats[0] -= nreads;
          pg.reset();  // (the halves' own families are theirs)
          for (DevBuf* b : {&small, &dist, &ext, &flag, &at, &acc, &k1, &v1, &k2, &v2, &rdist, &rext, &rflag, &rat}) b->release();
          MG_TRY(align_range(j, r0, mid));
          return align_range(j, mid, r1);
        }
        if (gap_list.alloc(nrefined * 4) != MG_OK || gap_ops.alloc(ops_bytes) != MG_OK)
          return fail(MG_ERR_NOMEM, "the %llu refined candidates of a batch (%llu bytes) do not fit on the device",
                      (unsigned long long)nrefined, (unsigned long long)need);
        MG_HIP(hipMemsetAsync(d_cursor + 4, 0, 2 * sizeof(uint64_t), st));
        hipLaunchKernelGGL(k_al_gap_mark<true>, dim3(al_grid(nacc_aln)), dim3(kAB), 0, st, acc.as<Accepted>(), nacc_aln, r0, j.d_offs,
                           j.gap.band, d_cursor + 4, gap_list.as<uint32_t>());
        MG_HIP(hipGetLastError());
        const uint32_t max_len = (uint32_t)g3[2];
        const unsigned grid = grid_cap(grid_for(nrefined, 1, (unsigned)c.num_cus * 32), "align_grid");
        hipLaunchKernelGGL(k_al_gap, dim3(grid), dim3(64), gap_lds_bytes(max_len, j.gap.band), st, gap_list.as<uint32_t>(), nrefined, r0,
                           j.d_bases, j.d_offs, j.ref->codes, ix->off.as<uint64_t>(), (int32_t)j.p.mismatch, (int32_t)j.gap.band,
                           (int32_t)j.gap.gap_open, (int32_t)j.gap.gap_extend, max_len, acc.as<Accepted>(), k1.as<uint64_t>(),
                           gap_ops.as<uint8_t>());
        MG_HIP(hipGetLastError());
      }
      j.stats[5] += nrefined;
    }
    if (!ps) ps.emplace("align_select");
    // stable, least significant part first: (a, pos0, strand, d), then (read, score descending)
    MG_TRY(sort_pairs_u64(k1.as<uint64_t>(), k2.as<uint64_t>(), v1.as<uint64_t>(), v2.as<uint64_t>(), nacc_aln, 52));
    hipLaunchKernelGGL(k_al_key2, dim3(al_grid(nacc_aln)), dim3(kAB), 0, st, acc.as<Accepted>(), v2.as<uint64_t>(), nacc_aln,
                       k1.as<uint64_t>());
    MG_HIP(hipGetLastError());
    MG_TRY(sort_pairs_u64(k1.as<uint64_t>(), k2.as<uint64_t>(), v2.as<uint64_t>(), v1.as<uint64_t>(), nacc_aln, 36));
  }
  j.stats[2] += ndist;
  j.stats[3] += nacc_aln;
  j.stats[6] += nresc;
  for (DevBuf* b : {&dist, &ext, &flag, &at, &rdist, &rext, &rflag, &rat}) b->release();
  // (k2: the sorted keys, v1: the alignments' indices in that order)
  DevBuf nkept, npool, rec_at, pool_at;
  MG_TRY(nkept.alloc(nreads * 4));
  MG_TRY(npool.alloc(nreads * 4));
  MG_TRY(rec_at.alloc((nreads + 1) * 8));
  MG_TRY(pool_at.alloc((nreads + 1) * 8));
  BatchOut none{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  const unsigned pair_grid = grid_cap(grid_for(nreads / 2, kPB, (unsigned)c.num_cus * 8), "align_grid");
  if (paired)
    hipLaunchKernelGGL(k_al_select_pair<false>, dim3(pair_grid), dim3(kPB), 0, st, acc.as<Accepted>(), k2.as<uint64_t>(), v1.as<uint64_t>(),
                       nacc_aln, r0, nreads, j.d_bases, j.d_offs, gap_ops.as<uint8_t>(), j.p.max_secondary, j.p.sec_pct, j.pairs.max_insert,
                       nkept.as<uint32_t>(), npool.as<uint32_t>(), d_cursor + 2, d_cursor + 3, (const uint64_t*)nullptr,
                       (const uint64_t*)nullptr, none);
  else
    hipLaunchKernelGGL(k_al_select<false>, dim3(al_grid(nreads)), dim3(kAB), 0, st, acc.as<Accepted>(), k2.as<uint64_t>(), v1.as<uint64_t>(),
                       nacc_aln, r0, nreads, j.d_bases, j.d_offs, gap_ops.as<uint8_t>(), j.p.max_secondary, j.p.sec_pct, nkept.as<uint32_t>(),
                       npool.as<uint32_t>(), d_cursor + 2, (const uint64_t*)nullptr, (const uint64_t*)nullptr, none);
  MG_HIP(hipGetLastError());
  uint64_t nrec = 0, npool_bytes = 0, aligned = 0, proper = 0;
  MG_TRY(exclusive_sum_u32_to_u64(nkept.as<uint32_t>(), rec_at.as<uint64_t>(), nreads, &nrec));
  MG_TRY(exclusive_sum_u32_to_u64(npool.as<uint32_t>(), pool_at.as<uint64_t>(), nreads, &npool_bytes));
  MG_TRY(fetch_u64(d_cursor + 2, &aligned));
  if (paired) MG_TRY(fetch_u64(d_cursor + 3, &proper));
  j.stats[1] += aligned;
  j.stats[7] += proper;
  j.stats[4] += nrec;
  if (!nrec) return MG_OK;
  const uint64_t have = sb->nrecs, total = have + nrec;
  if (grow(sb->recs, have * sizeof(mg_aln_rec), total * sizeof(mg_aln_rec)) != MG_OK ||
      ((j.want & MG_BATCH_PLACES) && grow(sb->places, have * sizeof(mg_aln_place), total * sizeof(mg_aln_place)) != MG_OK) ||
      ((j.want & MG_BATCH_EDITS) && grow(sb->edits, have * sizeof(mg_aln_edit), total * sizeof(mg_aln_edit)) != MG_OK) ||
      ((j.want & MG_BATCH_BASES) && (grow(sb->bases, have * sizeof(mg_aln_bases), total * sizeof(mg_aln_bases)) != MG_OK ||
                                     grow(sb->pool, sb->npool, sb->npool + npool_bytes + 16) != MG_OK)))
    return fail(MG_ERR_NOMEM, "the %llu records of the reads aligned so far (%llu bytes) do not fit on the device",
                (unsigned long long)total, (unsigned long long)(total * 48));
  BatchOut out{sb->recs.as<mg_aln_rec>() + have,
               (j.want & MG_BATCH_PLACES) ? sb->places.as<mg_aln_place>() + have : nullptr,
               (j.want & MG_BATCH_EDITS) ? sb->edits.as<mg_aln_edit>() + have : nullptr,
               (j.want & MG_BATCH_BASES) ? sb->bases.as<mg_aln_bases>() + have : nullptr,
               (j.want & MG_BATCH_BASES) ? sb->pool.as<uint8_t>() : nullptr,
               sb->npool};
  if (paired)
    hipLaunchKernelGGL(k_al_select_pair<true>, dim3(pair_grid), dim3(kPB), 0, st, acc.as<Accepted>(), k2.as<uint64_t>(), v1.as<uint64_t>(),
                       nacc_aln, r0, nreads, j.d_bases, j.d_offs, gap_ops.as<uint8_t>(), j.p.max_secondary, j.p.sec_pct, j.pairs.max_insert,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                       rec_at.as<uint64_t>(), pool_at.as<uint64_t>(), out);
  else
    hipLaunchKernelGGL(k_al_select<true>, dim3(al_grid(nreads)), dim3(kAB), 0, st, acc.as<Accepted>(), k2.as<uint64_t>(), v1.as<uint64_t>(),
                       nacc_aln, r0, nreads, j.d_bases, j.d_offs, gap_ops.as<uint8_t>(), j.p.max_secondary, j.p.sec_pct, (uint32_t*)nullptr,
                       (uint32_t*)nullptr, (unsigned long long*)nullptr, rec_at.as<uint64_t>(), pool_at.as<uint64_t>(), out);
  MG_HIP(hipGetLastError());
  MG_HIP(hipStreamSynchronize(st));  // (the scratch of this batch goes back to the pool behind its kernels)
  sb->nrecs = total;
  if (j.want & MG_BATCH_BASES) sb->npool += npool_bytes;
  return MG_OK;
}

int check_params(const mg_align_params* p) {
  if (p->k < mga::kMinK || p->k > mga::kMaxK || p->k % 2 == 0) return fail(MG_ERR_ARG, "k = %u: odd and within 11 to 31", p->k);
  if (p->w < 1 || p->w > mga::kMaxW) return fail(MG_ERR_ARG, "w = %u: within 1 to 32", p->w);
  if (p->max_occ < 1 || p->max_occ > 65535) return fail(MG_ERR_ARG, "max_occ = %u: within 1 to 65535", p->max_occ);
  if (p->min_score < 1 || p->min_score > mga::kMaxRead) return fail(MG_ERR_ARG, "min_score = %u: within 1 to 1024", p->min_score);
  if (p->mismatch < 1 || p->mismatch > 64) return fail(MG_ERR_ARG, "mismatch = %u: within 1 to 64", p->mismatch);
  if (p->max_secondary > mga::kMaxSecondary) return fail(MG_ERR_ARG, "max_secondary = %u: within 0 to 15", p->max_secondary);
  if (p->sec_pct > 100) return fail(MG_ERR_ARG, "sec_pct = %u: within 0 to 100", p->sec_pct);
  return MG_OK;
}

int check_pairs(const mg_align_pairs* p) {
  if (p->interleaved > 1) return fail(MG_ERR_ARG, "interleaved = %u: 0 or 1", p->interleaved);
  if (p->max_insert < 1 || p->max_insert > mga::kMaxInsert) return fail(MG_ERR_ARG, "max_insert = %u: within 1 to 8192", p->max_insert);
  if (p->rescue > mga::kMaxRescue) return fail(MG_ERR_ARG, "rescue = %u: within 0 to 8", p->rescue);
  return MG_OK;
}

int check_gap(const mg_align_gap* g) {
  if (g->band > mga::kMaxBand) return fail(MG_ERR_ARG, "band = %u: within 0 to 31", g->band);
  if (g->gap_open > 64) return fail(MG_ERR_ARG, "gap_open = %u: within 0 to 64", g->gap_open);
  if (g->gap_extend < 1 || g->gap_extend > 64) return fail(MG_ERR_ARG, "gap_extend = %u: within 1 to 64", g->gap_extend);
  return MG_OK;
}

}  // namespace

extern "C" {

int mg_align_index_build(const mg_refseq* ref, uint32_t k, uint32_t w, mg_align_index** out) {
  MG_REQUIRE_READY();
  if (!ref || !out) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  if (k < mga::kMinK || k > mga::kMaxK || k % 2 == 0) return fail(MG_ERR_ARG, "k = %u: odd and within 11 to 31", k);
  if (w < 1 || w > mga::kMaxW) return fail(MG_ERR_ARG, "w = %u: within 1 to 32", w);
  Context& c = ctx();
  hipStream_t st = c.stream;
  std::unique_ptr<mg_align_index> h(new mg_align_index());
  h->k = k;
  h->w = w;
  h->nacc = ref->nacc;
  h->nsites = ref->nsites;
  std::vector<uint64_t> h_off(ref->nacc + 1ull, 0);
  uint64_t positions = 0;
  for (uint32_t a = 0; a < ref->nacc; ++a) {
    h_off[a + 1] = h_off[a] + ref->h_len[a];
    if (ref->h_len[a] >= k) positions += ref->h_len[a] - k + 1;
  }
  if (h->nsites + (ref->nacc + 2ull) * kPad >= (1ull << kStrandShift))
    return fail(MG_ERR_ARG, "%llu reference bases in %u accessions: the diagonals need more than 39 bits", (unsigned long long)h->nsites,
                ref->nacc);
  // by arithmetic, before anything is allocated or launched: 2 / (w + 1) of the positions are expected as entries, each 16 bytes
  // twice (unsorted and sorted) and 16 bytes of the radix sort's own
  const uint64_t expect = 2 * positions / (w + 1ull), need = expect * 48;
  uint64_t room = 0;
  MG_TRY(mem_room(&room));
  if (need > room)
    return fail(MG_ERR_NOMEM, "the aligner's index (%llu bytes for about %llu minimizers) does not fit on the device",
                (unsigned long long)need, (unsigned long long)expect);
  MG_TRY(h->off.alloc((ref->nacc + 1ull) * sizeof(uint64_t)));
  MG_HIP(hipMemcpyAsync(h->off.p, h_off.data(), (ref->nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipStreamSynchronize(st));
  ProfScope ps("align_index");
  DevBuf small;
  MG_TRY(small.alloc(2 * sizeof(uint64_t)));
  MG_HIP(hipMemsetAsync(small.p, 0, 2 * sizeof(uint64_t), st));
  unsigned long long* d_cursor = small.as<unsigned long long>();
  uint64_t nent = 0;
  const unsigned grid = grid_for(h->nsites, kAB, (unsigned)c.num_cus * 8);
  if (h->nsites && ref->nacc) {
    hipLaunchKernelGGL(k_al_ref<false>, dim3(grid), dim3(kAB), 0, st, ref->codes, h->off.as<uint64_t>(), ref->loaded.as<uint8_t>(),
                       (uint64_t)ref->nacc, h->nsites, k, w, d_cursor, (uint64_t*)nullptr, (uint64_t*)nullptr);
    MG_HIP(hipGetLastError());
    MG_TRY(fetch_u64(d_cursor, &nent));
  }
  h->nent = nent;
  if (nent > 0xfffffff0ull) return fail(MG_ERR_ARG, "%llu minimizers: the index holds fewer than 2^32", (unsigned long long)nent);
  if (nent) {
    DevBuf ukeys, uvals, rkeys, rcounts;
    if (ukeys.alloc(nent * 8) != MG_OK || uvals.alloc(nent * 8) != MG_OK || h->keys.alloc(nent * 8) != MG_OK ||
        h->vals.alloc(nent * 8) != MG_OK)
      return fail(MG_ERR_NOMEM, "the aligner's index (%llu bytes for %llu minimizers) does not fit on the device",
                  (unsigned long long)(nent * 48), (unsigned long long)nent);
    MG_HIP(hipMemsetAsync(d_cursor, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(k_al_ref<true>, dim3(grid), dim3(kAB), 0, st, ref->codes, h->off.as<uint64_t>(), ref->loaded.as<uint8_t>(),
                       (uint64_t)ref->nacc, h->nsites, k, w, d_cursor, ukeys.as<uint64_t>(), uvals.as<uint64_t>());
    MG_HIP(hipGetLastError());
    MG_TRY(sort_pairs_u64(ukeys.as<uint64_t>(), h->keys.as<uint64_t>(), uvals.as<uint64_t>(), h->vals.as<uint64_t>(), nent, 64));
    MG_HIP(hipStreamSynchronize(st));
    ukeys.release();
    uvals.release();
    // the unique keys: as many as entries at the most, trimmed to their number below
    if (rkeys.alloc(nent * 8) != MG_OK || rcounts.alloc(nent * 4) != MG_OK)
      return fail(MG_ERR_NOMEM, "the aligner's unique-key table (%llu bytes) does not fit on the device", (unsigned long long)(nent * 20));
    MG_TRY(rle_keys(h->keys.as<uint64_t>(), nent, rkeys.as<uint64_t>(), rcounts.as<uint32_t>(), small.as<uint64_t>() + 1));
    MG_TRY(fetch_u64(small.as<uint64_t>() + 1, &h->nuniq));
    if (h->ukey.alloc(h->nuniq * 8) != MG_OK || h->ucount.alloc(h->nuniq * 4) != MG_OK || h->ustart.alloc((h->nuniq + 1) * 8) != MG_OK)
      return fail(MG_ERR_NOMEM, "the aligner's unique-key table (%llu bytes) does not fit on the device",
                  (unsigned long long)(h->nuniq * 20));
    MG_HIP(hipMemcpyAsync(h->ukey.p, rkeys.p, h->nuniq * 8, hipMemcpyDeviceToDevice, st));
    MG_HIP(hipMemcpyAsync(h->ucount.p, rcounts.p, h->nuniq * 4, hipMemcpyDeviceToDevice, st));
    uint64_t total = 0;
    MG_TRY(exclusive_sum_u32_to_u64(h->ucount.as<uint32_t>(), h->ustart.as<uint64_t>(), h->nuniq, &total));  // (synchronises)
    if (total != nent) return fail(MG_ERR_STATE, "the unique-key table counts %llu entries of %llu", (unsigned long long)total,
                                   (unsigned long long)nent);
  } else {
    MG_HIP(hipStreamSynchronize(st));
  }
  *out = h.release();
  return MG_OK;
}

int mg_align_index_stats(const mg_align_index* ix, uint64_t out4[4]) {
  if (!ix || !out4) return fail(MG_ERR_ARG, "null argument");
  out4[0] = ix->nent;
  out4[1] = ix->nuniq;
  out4[2] = ix->k;
  out4[3] = ix->w;
  return MG_OK;
}

int mg_align_index_download(const mg_align_index* ix, uint64_t* keys, uint64_t* vals) {
  MG_REQUIRE_READY();
  if (!ix || (ix->nent && (!keys || !vals))) return fail(MG_ERR_ARG, "null argument");
  if (ix->nent) {
    MG_TRY(mg_memcpy_d2h(keys, ix->keys.p, ix->nent * 8));
    MG_TRY(mg_memcpy_d2h(vals, ix->vals.p, ix->nent * 8));
  }
  return MG_OK;
}

void mg_align_index_free(mg_align_index* ix) { delete ix; }

int mg_align_reads_dev(const mg_align_index* ix, const mg_refseq* ref, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t nreads,
                       const mg_align_params* params, unsigned want_mask, mg_sam_batch** batch, uint64_t stats5[5]) {
  const mg_align_gap off{0, 6, 1};
  uint64_t stats6[6];
  const int rc = mg_align_reads_gapped_dev(ix, ref, d_bases, d_offsets, nreads, params, &off, want_mask, batch, stats6);
  if (rc == MG_OK && stats5)
    for (int i = 0; i < 5; ++i) stats5[i] = stats6[i];
  return rc;
}

int mg_align_reads_gapped_dev(const mg_align_index* ix, const mg_refseq* ref, const uint8_t* d_bases, const uint64_t* d_offsets,
                              uint64_t nreads, const mg_align_params* params, const mg_align_gap* gap, unsigned want_mask,
                              mg_sam_batch** batch, uint64_t stats6[6]) {
  uint64_t stats8[8];
  const int rc = mg_align_reads_paired_dev(ix, ref, d_bases, d_offsets, nreads, params, gap, nullptr, want_mask, batch, stats8);
  if (rc == MG_OK && stats6)
    for (int i = 0; i < 6; ++i) stats6[i] = stats8[i];
  return rc;
}

int mg_align_reads_paired_dev(const mg_align_index* ix, const mg_refseq* ref, const uint8_t* d_bases, const uint64_t* d_offsets,
                              uint64_t nreads, const mg_align_params* params, const mg_align_gap* gap, const mg_align_pairs* pairs,
                              unsigned want_mask, mg_sam_batch** batch, uint64_t stats8[8]) {
  MG_REQUIRE_READY();
  if (!ix || !ref || !params || !gap || !batch || (nreads && (!d_bases || !d_offsets))) return fail(MG_ERR_ARG, "null argument");
  MG_TRY(check_params(params));
  MG_TRY(check_gap(gap));
  mg_align_pairs pp{0, 1000, 0};  // (no pairs: the other fields are not read)
  if (pairs && pairs->interleaved) {
    MG_TRY(check_pairs(pairs));
    if (nreads % 2) return fail(MG_ERR_ARG, "%llu reads: interleaved pairs are an even number", (unsigned long long)nreads);
    pp = *pairs;
  }
  if (params->k != ix->k || params->w != ix->w)
    return fail(MG_ERR_ARG, "the index was built for k = %u, w = %u, not %u, %u", ix->k, ix->w, params->k, params->w);
  if (ref->nacc != ix->nacc || ref->nsites != ix->nsites) return fail(MG_ERR_ARG, "the index was built for another reference");
  if (want_mask & ~(MG_BATCH_PLACES | MG_BATCH_EDITS | MG_BATCH_BASES))
    return fail(MG_ERR_ARG, "an aligned batch carries places, edits and bases only: it is neither keyed nor named");
  if (reinterpret_cast<uintptr_t>(d_bases) & 7u) return fail(MG_ERR_ARG, "the reads' bases must be 8-byte aligned");
  std::unique_ptr<mg_sam_batch> fresh;
  mg_sam_batch* sb = *batch;
  if (!sb) {
    fresh.reset(new mg_sam_batch());
    sb = fresh.get();
    MG_TRY(sb->recs.alloc(256));
    sb->placed = (want_mask & MG_BATCH_PLACES) != 0;
    sb->edited = (want_mask & MG_BATCH_EDITS) != 0;
    sb->based = (want_mask & MG_BATCH_BASES) != 0;
    if (sb->placed) MG_TRY(sb->places.alloc(256));
    if (sb->edited) MG_TRY(sb->edits.alloc(256));
    if (sb->based) {
      MG_TRY(sb->bases.alloc(256));
      MG_TRY(sb->pool.alloc(256));
    }
  } else if (sb->keyed || sb->named || sb->placed != ((want_mask & MG_BATCH_PLACES) != 0) ||
             sb->edited != ((want_mask & MG_BATCH_EDITS) != 0) || sb->based != ((want_mask & MG_BATCH_BASES) != 0)) {
    return fail(MG_ERR_STATE, "the batch to append to carries other side arrays than this call asks for");
  }
  AlignJob j{ix, ref, d_bases, d_offsets, *params, *gap, pp, want_mask, sb};
  if (nreads) MG_TRY(align_range(j, 0, nreads));  // (on failure a fresh batch goes; one handed in keeps what it had)
  else j.stats[0] = 0;
  if (stats8)
    for (int i = 0; i < 8; ++i) stats8[i] = j.stats[i];
  if (fresh) *batch = fresh.release();
  return MG_OK;
}

}  // extern "C"
