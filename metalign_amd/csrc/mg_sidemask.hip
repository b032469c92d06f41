// mg_sidemask.hip — the records a side output counts under --side_reads unique (metalign_amd/side_reads.py is the definition;
// mg_sidemask_core.h the per-record decision).
//
// A record's read is the number of NEW bits at or before it, so the join of stage C's verdict words back to the records is a prefix
// sum over the stream.  Three launches, none of which waits on another workgroup:
//
//   k_mask_count   NEW bits per tile of mgs::kTile records: a ballot and a popcount per wavefront and 64 records.
//   k_mask_scan    the exclusive scan of the tile counts by one workgroup (mg_side_dev.h: block_scan_excl), in 64 bits,
//                  on top of the carry of the launches before it (a call above 2^31 records is cut into several).
//   k_mask_apply   a workgroup per tile, a wavefront per quarter of it, the records held in registers: the ordinal is the tile's base,
//                  the wavefronts before it, the 64-record steps before it and mbcnt over the step's ballot; then word 0 of the read
//                  (and of the read before it for a NEW record) is gathered and out[i] = recs[i], with FLAG bit 2048 set where the
//                  record is masked.  16-byte loads and stores; every record is read and written by the same lane, all loads before
//                  the first store, so out may be recs.
//
// Per record: 16 B read twice, 16 B written, and 8 to 16 B of verdict words (mostly shared between the lanes of a wavefront).
#include "mg_internal.h"
#include "mg_sidemask_core.h"
#include "mg_side_dev.h"

using namespace mg;

namespace {

constexpr unsigned kBlock = 256, kWaves = kBlock / 64, kPerWave = mgs::kTile / kWaves, kSteps = kPerWave / 64, kScanBlock = 256;
static_assert(kSteps * 64 * kWaves == mgs::kTile && kLaunchMax % mgs::kTile == 0, "tile shape");

struct Word0 {  // word 0 of read r
  const unsigned long long* a;
  __device__ __forceinline__ uint64_t operator[](uint64_t r) const { return a[2 * r]; }
};

__global__ __launch_bounds__(kBlock) void k_mask_count(const mg_aln_rec* __restrict__ recs, uint64_t n,
                                                       unsigned long long* __restrict__ tile_cnt) {
  __shared__ uint32_t s_w[kWaves];
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * mgs::kTile + (uint64_t)wv * kPerWave + lane;
  uint32_t cnt = 0;
#pragma unroll
  for (unsigned k = 0; k < kSteps; ++k) {
    const uint64_t i = first + 64ull * k;
    const bool nw = i < n && (recs[i].ref_new & MG_REC_NEW_BIT);
    cnt += (uint32_t)__builtin_popcountll(__ballot(nw));
  }
  if (lane == 0) s_w[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
    for (unsigned w = 0; w < kWaves; ++w) all += s_w[w];
    tile_cnt[blockIdx.x] = all;
  }
}

// t[i] = *carry + the counts before tile i; *carry += all of them
__global__ __launch_bounds__(kScanBlock) void k_mask_scan(unsigned long long* __restrict__ t, uint64_t ntiles,
                                                          unsigned long long* __restrict__ carry_io) {
  // (every thread reads the carry; it is written back behind the scan's barriers)
  const unsigned long long carry = block_scan_excl<unsigned long long, kScanBlock, 1>(t, ntiles, *carry_io);
  if (threadIdx.x == 0) *carry_io = carry;
}

// (recs and out may be the same array: no __restrict__ on them)
__global__ __launch_bounds__(kBlock) void k_mask_apply(const mg_aln_rec* recs, uint64_t n, const unsigned long long* __restrict__ tile_base,
                                                       const unsigned long long* __restrict__ assign, uint64_t nreads,
                                                       const uint32_t* __restrict__ ref2tax, uint32_t nref, mg_aln_rec* out,
                                                       unsigned long long* __restrict__ stats2) {
  __shared__ uint32_t s_w[kWaves];
  __shared__ unsigned long long s_kept, s_outside;
  const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * mgs::kTile + (uint64_t)wv * kPerWave + lane;
  const uint4* in4 = reinterpret_cast<const uint4*>(recs);
  uint4* out4 = reinterpret_cast<uint4*>(out);
  uint4 v[kSteps];
  unsigned long long nb[kSteps];
#pragma unroll
  for (unsigned k = 0; k < kSteps; ++k) {
    const uint64_t i = first + 64ull * k;
    v[k] = i < n ? in4[i] : make_uint4(0u, 0u, 0u, 0u);  // (a record behind the end is not NEW)
  }
  uint32_t cnt = 0;
#pragma unroll
  for (unsigned k = 0; k < kSteps; ++k) {
    nb[k] = __ballot((v[k].x & MG_REC_NEW_BIT) != 0);
    cnt += (uint32_t)__builtin_popcountll(nb[k]);
  }
  if (lane == 0) s_w[wv] = cnt;
  if (threadIdx.x == 0) { s_kept = 0; s_outside = 0; }
  __syncthreads();
  uint64_t base = tile_base[blockIdx.x];  // the NEW bits before this wavefront's records
  for (unsigned w = 0; w < wv; ++w) base += s_w[w];
  const Word0 w0{assign};
  uint32_t kept = 0, outside = 0;
#pragma unroll
  for (unsigned k = 0; k < kSteps; ++k) {
    const uint64_t i = first + 64ull * k;
    const bool live = i < n;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(nb[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nb[k], 0u));
    // the NEW bits in [0, i], minus one: 2^64 - 1 in front of the stream's first NEW record
    const uint64_t ord = base + below + (uint64_t)((nb[k] >> lane) & 1ull) - 1ull;
    mg_aln_rec r;
    r.ref_new = v[k].x; r.matched = v[k].y; r.total = v[k].z; r.flag_len = v[k].w;
    const bool kp = live && mgs::keep(r, ord, nreads, w0, ref2tax, nref);
    const bool outs = live && !mgs::in_range(ord, nreads);
    if (live) {
      if (!kp) v[k].w |= mgs::kMaskFlag;
      out4[i] = v[k];
    }
    kept += (uint32_t)__builtin_popcountll(__ballot(kp));
    outside += (uint32_t)__builtin_popcountll(__ballot(outs));
    base += (uint64_t)__builtin_popcountll(nb[k]);
  }
  if (lane == 0) {
    if (kept) atomicAdd(&s_kept, (unsigned long long)kept);
    if (outside) atomicAdd(&s_outside, (unsigned long long)outside);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_kept) atomicAdd(&stats2[0], s_kept);
    if (s_outside) atomicAdd(&stats2[1], s_outside);
  }
}

}  // namespace

extern "C" {

int mg_records_mask_unique_dev(const mg_aln_rec* d_recs, uint64_t n, const uint64_t* d_assign, uint64_t nreads, const uint32_t* d_ref2tax,
                               uint32_t nref, mg_aln_rec* d_out, uint64_t* d_stats2) {
  MG_REQUIRE_READY();
  if (!d_stats2 || (n && (!d_recs || !d_out)) || (nreads && !d_assign) || (nref && !d_ref2tax)) return fail(MG_ERR_ARG, "null argument");
  if ((((uintptr_t)d_recs) | ((uintptr_t)d_out)) & 15u) return fail(MG_ERR_ARG, "the records are not 16-byte aligned");
  if (n == 0) return MG_OK;
  ProfScope ps("sidemask");
  MG_TRY(mg_stage_c_join());  // (the verdict words are written on stage C's stream)
  hipStream_t st = ctx().stream;
  const uint64_t most = n < kLaunchMax ? n : kLaunchMax;
  const uint64_t max_tiles = (most + mgs::kTile - 1) / mgs::kTile;
  DevBuf tiles;  // u64[1 + tiles of a launch]: the carry of the ordinals, then the tile counts / bases
  MG_TRY(tiles.alloc((max_tiles + 1) * sizeof(uint64_t)));
  unsigned long long* carry = tiles.as<unsigned long long>();
  unsigned long long* tile = carry + 1;
  MG_HIP(hipMemsetAsync(carry, 0, sizeof(uint64_t), st));
  for (uint64_t at = 0; at < n; at += kLaunchMax) {
    const uint64_t m = n - at < kLaunchMax ? n - at : kLaunchMax;
    const unsigned ntiles = (unsigned)((m + mgs::kTile - 1) / mgs::kTile);
    hipLaunchKernelGGL(k_mask_count, dim3(ntiles), dim3(kBlock), 0, st, d_recs + at, m, tile);
    MG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(kScanBlock), 0, st, tile, (uint64_t)ntiles, carry);
    MG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mask_apply, dim3(ntiles), dim3(kBlock), 0, st, d_recs + at, m, (const unsigned long long*)tile,
                       reinterpret_cast<const unsigned long long*>(d_assign), nreads, d_ref2tax, nref, d_out + at,
                       reinterpret_cast<unsigned long long*>(d_stats2));
    MG_HIP(hipGetLastError());
  }
  return MG_OK;
}

}  // extern "C"
