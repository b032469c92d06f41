// mg_bam.hip — BAM alignment records (SAM specification §4) in HBM -> the same 16-byte records as their SAM text gives
// (mg_ingest.hip's tokeniser), so that a stored BAM goes to stage C without `samtools view` in front of it.
//
// A BAM record's start is known only from the previous record's block_size: the records of a piece form a chain.  The chain
// is found in parallel the way mg_inflate.hip finds deflate blocks — speculatively, then stitched:
//
//   k_bam_walk     the piece in chunks of kBamChunk bytes, one wavefront per chunk: the 64 lanes test 64 offsets at a time
//                  for a plausible record start (mg_bam_core.h: check), the first one is the chunk's speculative entry, and
//                  one lane walks the block_size chain from there to the chunk's end (the record offsets into the chunk's
//                  slots, the exit offset).  A chunk of short-read records holds ~13 of them: a dozen dependent loads per
//                  wavefront, hidden behind the other chunks' wavefronts (16 per CU for a 16 MB piece).
//   k_bam_stitch   chunk j's true entry is chunk j - 1's exit.  One workgroup compares 1024 chunks per step; a chunk whose
//                  speculative entry differs is walked again, in order, from its true entry — rare (a plausible start inside
//                  a record's bytes), and what makes the result exact whatever the data.  The end of the last complete
//                  record is what the piece consumed; a record that is not one on the true chain is a corrupt file.
//   scan + k_bam_compact   the record offsets, dense and in file order;
//   k_bam_decode   one lane per record (mg_bam_core.h: decode) -> LineOut, as k_sam_parse leaves a line;
//   then the SAM tokeniser's own k_sam_list / k_sam_emit / k_sam_last_qname (aln_emit_retained): the new-read bit and the
//   QNAME carried to the next piece.
//
// A BAM READS file (stages A / B) takes the same chain (bam_chain_dev), then:
//   k_bam_seq_len     one lane per record: its kept length (mg_bam_core.h: kept_len) and whether it is a read; two scans give
//                     every read's rank and its first base's place;
//   k_bam_seq_unpack  one wavefront per record: the 4-bit SEQ -> ASCII bases (reverse-complemented for 0x10) in a `bases +
//                     offsets` batch laid out like mg_reads_parse's, which the stage-A kernels take as they are.
#include <zlib.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mg_internal.h"
#include "mg_bam_core.h"

namespace mg {

constexpr uint32_t kBamChunk = 4096;                             // bytes of a piece per wavefront of k_bam_walk
constexpr uint32_t kBamCap = kBamChunk / mgb::kMinRecord + 2;    // record slots per chunk
constexpr int kBamWaves = 4;                                     // wavefronts per workgroup of k_bam_walk
constexpr uint64_t kNoEntry = ~0ull;

__global__ __launch_bounds__(64 * kBamWaves) void k_bam_walk(const uint8_t* __restrict__ b, uint64_t n, int32_t n_ref, uint64_t nchunks,
                                                             uint64_t* __restrict__ entry, uint64_t* __restrict__ exit,
                                                             uint32_t* __restrict__ count, uint32_t* __restrict__ status,
                                                             uint32_t* __restrict__ offs) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t j = (uint64_t)blockIdx.x * kBamWaves + threadIdx.x / 64; j < nchunks; j += (uint64_t)gridDim.x * kBamWaves) {
    const uint64_t cs = j * kBamChunk;
    const uint64_t ce = n - cs < kBamChunk ? n : cs + kBamChunk;
    uint64_t e = kNoEntry;
    if (j == 0) {
      e = 0;  // a piece starts at a record start
    } else {
      for (uint64_t q0 = cs; q0 < ce; q0 += 64) {
        const uint64_t q = q0 + lane;
        uint64_t nx = 0;
        const bool ok = q < ce && mgb::check(b, n, q, n_ref, &nx) == mgb::kOk;
        const uint64_t m = __ballot(ok);
        if (m) { e = q0 + (uint64_t)(__ffsll((unsigned long long)m) - 1); break; }
      }
    }
    if (lane == 0) {
      uint64_t x = ce;
      int st = mgb::kOk;
      uint32_t c = 0;
      if (e != kNoEntry) c = mgb::walk(b, n, n_ref, e, ce, cs, offs + j * kBamCap, kBamCap, &x, &st);
      entry[j] = e;
      exit[j] = x;
      count[j] = c;
      status[j] = (uint32_t)st;
    }
  }
}

// One workgroup.  res[0] = the end of the last complete record, res[1] = the offset of a non-record on the true chain (~0: none).
__global__ __launch_bounds__(1024) void k_bam_stitch(const uint8_t* __restrict__ b, uint64_t n, int32_t n_ref, uint64_t nchunks,
                                                     uint64_t* __restrict__ entry, uint64_t* __restrict__ exit,
                                                     uint32_t* __restrict__ count, uint32_t* __restrict__ status,
                                                     uint32_t* __restrict__ offs, unsigned long long* __restrict__ res) {
  __shared__ unsigned long long s_first;
  __shared__ uint64_t s_expect, s_next, s_bad;
  uint64_t j = 0;  // chunks before j are settled; s_expect = chunk j's true entry
  if (threadIdx.x == 0) { s_expect = 0; s_bad = kNoEntry; }
  __syncthreads();
  while (j < nchunks) {
    if (threadIdx.x == 0) s_first = kNoEntry;
    __syncthreads();
    const uint64_t expect0 = s_expect;
    const uint64_t k = j + threadIdx.x;
    if (k < nchunks) {
      const uint64_t want = threadIdx.x == 0 ? expect0 : exit[k - 1];
      if (entry[k] != want || status[k] == (uint32_t)mgb::kBad) atomicMin(&s_first, (unsigned long long)k);
    }
    __syncthreads();
    const uint64_t f = s_first;
    if (f == kNoEntry) {
      j = nchunks - j < blockDim.x ? nchunks : j + blockDim.x;
      __syncthreads();
      if (threadIdx.x == 0) s_expect = exit[j - 1];
      __syncthreads();
      continue;
    }
    if (threadIdx.x == 0) {
      uint64_t want = f == j ? expect0 : exit[f - 1];
      uint64_t c = f;
      while (c < nchunks) {
        if (entry[c] == want) {  // back on the speculative chain (or the chunk's own walk met a non-record)
          if (status[c] == (uint32_t)mgb::kBad) s_bad = exit[c];
          break;
        }
        const uint64_t cs = c * kBamChunk;
        const uint64_t ce = n - cs < kBamChunk ? n : cs + kBamChunk;
        uint64_t x = want;
        int st = mgb::kOk;
        count[c] = mgb::walk(b, n, n_ref, want, ce, cs, offs + c * kBamCap, kBamCap, &x, &st);
        entry[c] = want;
        exit[c] = x;
        status[c] = (uint32_t)st;
        if (st == mgb::kBad) { s_bad = x; break; }
        want = x;
        ++c;
      }
      s_next = c;
      s_expect = want;
    }
    __syncthreads();
    if (s_bad != kNoEntry) break;
    j = s_next;
  }
  if (threadIdx.x == 0) {
    res[0] = nchunks ? exit[nchunks - 1] : 0;
    res[1] = s_bad;
  }
}

// one wavefront per chunk: its record offsets -> their places in file order
__global__ __launch_bounds__(256) void k_bam_compact(const uint32_t* __restrict__ count, const uint64_t* __restrict__ rank,
                                                     const uint32_t* __restrict__ offs, uint64_t nchunks, uint64_t* __restrict__ rec_off) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t j = (uint64_t)blockIdx.x * 4 + threadIdx.x / 64; j < nchunks; j += (uint64_t)gridDim.x * 4) {
    const uint32_t c = count[j];
    const uint64_t at = rank[j];
    for (uint32_t i = lane; i < c; i += 64) rec_off[at + i] = j * kBamChunk + offs[j * kBamCap + i];
  }
}

// one lane per record; err: [0] = first failing record (atomicMin), kinds[record] its kind
__global__ __launch_bounds__(256) void k_bam_decode(const uint8_t* __restrict__ b, uint64_t n, const uint64_t* __restrict__ rec_off,
                                                    uint64_t nrec, const int32_t* __restrict__ refmap, int32_t n_ref,
                                                    LineOut* __restrict__ out, uint32_t* __restrict__ retained,
                                                    unsigned long long* __restrict__ err, uint32_t* __restrict__ err_kind) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; r < nrec; r += stride) {
    mgb::Decoded d;
    mgb::decode(b, n, rec_off[r], refmap, n_ref, &d);
    LineOut o;
    o.rec = d.rec;
    o.qbeg = d.qbeg;
    o.qlen = d.qlen;
    o.retained = d.retained;
    out[r] = o;
    retained[r] = d.retained;
    if (d.kind != mgb::kNone) {
      atomicMin(err, (unsigned long long)r);
      err_kind[r] = d.kind;
    }
  }
}

// The chain step shared by the SAM-record decoder and the reads path: walk -> stitch -> scan -> compact.  nbytes > 0.
// -> *d_rec_off (scratch: the record offsets, dense and in file order), *nrec, *consumed = the end of the last complete record.
// A non-record on the true chain, or (final) bytes after the last complete record: MG_ERR_ARG, *err_at = that byte of the piece.
static int bam_chain_dev(const uint8_t* d_bytes, uint64_t nbytes, int32_t n_ref, bool final, uint64_t* consumed, uint64_t** d_rec_off,
                         uint64_t* nrec_out, uint64_t* err_at) {
  Context& c = ctx();
  hipStream_t st = c.stream;
  *d_rec_off = nullptr;
  *nrec_out = 0;
  const uint64_t nchunks = (nbytes + kBamChunk - 1) / kBamChunk;
  uint64_t* d_entry = (uint64_t*)scratch("bam_entry", nchunks * sizeof(uint64_t));
  uint64_t* d_exit = (uint64_t*)scratch("bam_exit", nchunks * sizeof(uint64_t));
  uint32_t* d_count = (uint32_t*)scratch("bam_count", nchunks * sizeof(uint32_t));
  uint32_t* d_status = (uint32_t*)scratch("bam_status", nchunks * sizeof(uint32_t));
  uint32_t* d_offs = (uint32_t*)scratch("bam_offs", nchunks * kBamCap * sizeof(uint32_t));
  uint64_t* d_crank = (uint64_t*)scratch("bam_crank", (nchunks + 1) * sizeof(uint64_t));
  unsigned long long* d_res = (unsigned long long*)scratch("bam_res", 4 * sizeof(unsigned long long));
  if (!d_entry || !d_exit || !d_count || !d_status || !d_offs || !d_crank || !d_res) return MG_ERR_NOMEM;
  uint64_t* pin = host_words();
  uint64_t nrec = 0, end = 0, bad = 0;
  {
    ProfScope ps("bam_chain");
    hipLaunchKernelGGL(k_bam_walk, dim3(grid_for(nchunks, kBamWaves, (unsigned)c.num_cus * 64)), dim3(64 * kBamWaves), 0, st, d_bytes,
                       nbytes, n_ref, nchunks, d_entry, d_exit, d_count, d_status, d_offs);
    hipLaunchKernelGGL(k_bam_stitch, dim3(1), dim3(1024), 0, st, d_bytes, nbytes, n_ref, nchunks, d_entry, d_exit, d_count, d_status,
                       d_offs, d_res);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(pin + 40, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));  // (rides on the scan's synchronisation)
    MG_TRY(exclusive_sum_u32_to_u64(d_count, d_crank, nchunks, &nrec));
    end = reinterpret_cast<const volatile uint64_t*>(pin)[40];
    bad = reinterpret_cast<const volatile uint64_t*>(pin)[41];
  }
  if (bad != kNoEntry) {
    *err_at = bad;
    return fail(MG_ERR_ARG, "BAM: no record at byte %llu of the piece (a corrupt block_size?)", (unsigned long long)bad);
  }
  if (final && end != nbytes) {
    *err_at = end;
    return fail(MG_ERR_ARG, "BAM: truncated record at byte %llu of the last piece", (unsigned long long)end);
  }
  if (consumed) *consumed = end;
  if (nrec) {
    uint64_t* d_off = (uint64_t*)scratch("bam_recoff", nrec * sizeof(uint64_t));
    if (!d_off) return MG_ERR_NOMEM;
    hipLaunchKernelGGL(k_bam_compact, dim3(grid_for(nchunks, 4, (unsigned)c.num_cus * 16)), dim3(256), 0, st, d_count, d_crank, d_offs,
                       nchunks, d_off);
    MG_HIP(hipGetLastError());
    *d_rec_off = d_off;
  }
  *nrec_out = nrec;
  return MG_OK;
}

int bam_tokenize_prefix_dev(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* d_refmap, int32_t n_ref, const char* prev_qname,
                            bool final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec, bool keyed, bool named,
                            bool placed, bool edited, bool based) {
  MG_REQUIRE_READY();
  if (!out || !d_refmap) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  if (err_kind) *err_kind = 0;
  if (err_rec) *err_rec = 0;
  if (consumed) *consumed = 0;
  if (nbytes && !d_bytes) return fail(MG_ERR_ARG, "null device bytes");
  Context& c = ctx();
  hipStream_t st = c.stream;
  std::unique_ptr<mg_sam_batch> sb(new mg_sam_batch());
  if (prev_qname) sb->last_qname = prev_qname;
  sb->keyed = keyed;
  if (keyed) MG_TRY(sb->keys.alloc(16));  // (replaced by aln_emit_retained's when there are records)
  if (nbytes == 0) {
    MG_TRY(sb->recs.alloc(16));
    if (named) MG_TRY(names_empty(sb.get()));
    if (placed) MG_TRY(places_empty(sb.get()));
    if (edited) MG_TRY(edits_empty(sb.get()));
    if (based) MG_TRY(bases_empty(sb.get()));
    *out = sb.release();
    return MG_OK;
  }
  uint64_t* d_off = nullptr;
  uint64_t nrec = 0, at = 0;
  {
    const int rc = bam_chain_dev(d_bytes, nbytes, n_ref, final, consumed, &d_off, &nrec, &at);
    if (rc == MG_ERR_ARG) {
      if (err_kind) *err_kind = (int)mgb::kCorrupt;
      if (err_rec) *err_rec = at;
    }
    MG_TRY(rc);
  }
  unsigned long long* d_res = (unsigned long long*)scratch("bam_res", 4 * sizeof(unsigned long long));
  uint64_t* pin = host_words();
  const size_t plen = prev_qname ? strlen(prev_qname) : 0;
  uint8_t* d_prev = (uint8_t*)scratch("bam_prev", plen + 16);
  if (!d_prev || !d_res) return MG_ERR_NOMEM;
  if (plen) MG_HIP(hipMemcpyAsync(d_prev, prev_qname, plen, hipMemcpyHostToDevice, st));
  uint64_t nret = 0;
  if (nrec) {
    ProfScope ps("bam_decode");
    LineOut* d_lines = (LineOut*)scratch("bam_lines", nrec * sizeof(LineOut));
    uint32_t* d_ret = (uint32_t*)scratch("bam_ret", nrec * sizeof(uint32_t));
    uint64_t* d_rank = (uint64_t*)scratch("bam_rank", (nrec + 1) * sizeof(uint64_t));
    uint32_t* d_kind = (uint32_t*)scratch("bam_kind", nrec * sizeof(uint32_t));
    if (!d_lines || !d_ret || !d_rank || !d_kind) return MG_ERR_NOMEM;
    MG_HIP(hipMemsetAsync(d_res + 2, 0xff, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_bam_decode, dim3(grid_for(nrec, 256, (unsigned)c.num_cus * 16)), dim3(256), 0, st, d_bytes, nbytes, d_off, nrec,
                       d_refmap, n_ref, d_lines, d_ret, d_res + 2, d_kind);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(pin + 42, d_res + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_TRY(exclusive_sum_u32_to_u64(d_ret, d_rank, nrec, &nret));
    const uint64_t h_err = reinterpret_cast<const volatile uint64_t*>(pin)[42];
    if (h_err != kNoEntry) {
      uint32_t kind = 0;
      MG_HIP(hipMemcpyAsync(&kind, d_kind + h_err, sizeof(kind), hipMemcpyDeviceToHost, st));
      MG_HIP(hipStreamSynchronize(st));
      if (err_kind) *err_kind = (int)kind;
      if (err_rec) *err_rec = h_err;
      return fail(MG_ERR_ARG, "BAM record %llu of the piece: %s (kind %u)", (unsigned long long)h_err,
                  kind == mgb::kCorrupt ? "corrupt, or a CIGAR kept in a CG tag (not supported)" : "not decided on the device", kind);
    }
    // (placed: pos and the ops M, D, N, X of the record body — k_bam_place, beside the other steps over the emitted records)
    MG_TRY(aln_emit_retained(d_bytes, d_lines, d_ret, d_rank, nrec, nret, d_prev, (uint32_t)plen, sb.get(), keyed, named,
                             placed ? kPlaceBam : kPlaceNone, nullptr, edited ? kPlaceBam : kPlaceNone, nullptr,
                             based ? kPlaceBam : kPlaceNone));
  } else {
    MG_TRY(sb->recs.alloc(16));
    if (named) MG_TRY(names_empty(sb.get()));
    if (placed) MG_TRY(places_empty(sb.get()));
    if (edited) MG_TRY(edits_empty(sb.get()));
    if (based) MG_TRY(bases_empty(sb.get()));
  }
  sb->nrecs = nret;
  *out = sb.release();
  return MG_OK;
}

// ---- reads (stages A / B): BAM records -> bases + offsets as mg_reads_parse leaves them (mg_bam_core.h: seq_kept / seq_base) ----

// one lane per record: its kept length, and whether it is a read at all
__global__ __launch_bounds__(256) void k_bam_seq_len(const uint8_t* __restrict__ b, const uint64_t* __restrict__ rec_off, uint64_t nrec,
                                                     uint32_t* __restrict__ len, uint32_t* __restrict__ keep) {
  uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; r < nrec; r += stride) {
    uint32_t k = 0;
    len[r] = mgb::kept_len(b, rec_off[r], &k);
    keep[r] = k;
  }
}

// One wavefront per record: lane i writes bases 2i and 2i + 1 (+ 128 per step) of the read — consecutive output bytes across the
// wavefront whichever the strand (a reverse record reads its packed bytes backwards); pos[r] may be odd, the stores are bytes.
// offsets[rank[r]] = pos[r] for a read, and the last record closes the list: offsets[rank[nrec]] = pos[nrec].
constexpr int kUnpackWaves = 4;
__global__ __launch_bounds__(64 * kUnpackWaves) void k_bam_seq_unpack(const uint8_t* __restrict__ b, const uint64_t* __restrict__ rec_off,
                                                                      uint64_t nrec, const uint32_t* __restrict__ keep,
                                                                      const uint64_t* __restrict__ rank, const uint64_t* __restrict__ pos,
                                                                      uint8_t* __restrict__ bases, uint64_t* __restrict__ offsets) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t r = (uint64_t)blockIdx.x * kUnpackWaves + threadIdx.x / 64; r < nrec; r += (uint64_t)gridDim.x * kUnpackWaves) {
    if (lane == 0) {
      if (keep[r]) offsets[rank[r]] = pos[r];
      if (r == nrec - 1) offsets[rank[nrec]] = pos[nrec];
    }
    const uint64_t o = pos[r];
    const uint32_t len = (uint32_t)(pos[r + 1] - o);  // (0 for a record that is not a read)
    if (len == 0) continue;
    uint64_t seq = 0;
    uint32_t lseq = 0, flag = 0;
    mgb::seq_span(b, rec_off[r], &seq, &lseq, &flag);
    const bool rev = (flag & mgb::kFlagReverse) != 0;
    for (uint32_t j = 2 * lane; j < len; j += 128) {
      bases[o + j] = mgb::seq_base(b, seq, len, rev, j);
      if (j + 1 < len) bases[o + j + 1] = mgb::seq_base(b, seq, len, rev, j + 1);
    }
  }
}

int bam_reads_prefix_dev(const uint8_t* d_bytes, uint64_t nbytes, int32_t n_ref, bool final, uint64_t* consumed, mg_reads** out,
                         uint64_t* err_at) {
  MG_REQUIRE_READY();
  if (!out) return fail(MG_ERR_ARG, "null out handle");
  *out = nullptr;
  if (consumed) *consumed = 0;
  if (err_at) *err_at = 0;
  if (nbytes && !d_bytes) return fail(MG_ERR_ARG, "null device bytes");
  if (n_ref < 0) return fail(MG_ERR_ARG, "n_ref < 0");
  Context& c = ctx();
  hipStream_t st = c.stream;
  std::unique_ptr<mg_reads> rd(new mg_reads());
  uint64_t* d_off = nullptr;
  uint64_t nrec = 0, at = 0;
  if (nbytes) {
    const int rc = bam_chain_dev(d_bytes, nbytes, n_ref, final, consumed, &d_off, &nrec, &at);
    if (rc == MG_ERR_ARG && err_at) *err_at = at;
    MG_TRY(rc);
  }
  if (nrec == 0) {
    MG_TRY(rd->offsets.alloc(2 * sizeof(uint64_t)));
    MG_TRY(rd->bases.alloc(16));
    MG_HIP(hipMemsetAsync(rd->offsets.p, 0, 2 * sizeof(uint64_t), st));
    *out = rd.release();
    return MG_OK;
  }
  uint32_t* d_len = (uint32_t*)scratch("bamr_len", nrec * sizeof(uint32_t));
  uint32_t* d_keep = (uint32_t*)scratch("bamr_keep", nrec * sizeof(uint32_t));
  uint64_t* d_rank = (uint64_t*)scratch("bamr_rank", (nrec + 1) * sizeof(uint64_t));
  uint64_t* d_pos = (uint64_t*)scratch("bamr_pos", (nrec + 1) * sizeof(uint64_t));
  if (!d_len || !d_keep || !d_rank || !d_pos) return MG_ERR_NOMEM;
  ProfScope ps("bam_reads");
  hipLaunchKernelGGL(k_bam_seq_len, dim3(grid_for(nrec, 256, (unsigned)c.num_cus * 16)), dim3(256), 0, st, d_bytes, d_off, nrec, d_len,
                     d_keep);
  MG_HIP(hipGetLastError());
  uint64_t nkept = 0;
  MG_TRY(exclusive_sum_u32_to_u64(d_keep, d_rank, nrec, &nkept));
  MG_TRY(exclusive_sum_u32_to_u64(d_len, d_pos, nrec, &rd->nbases));
  rd->nreads = nkept;
  MG_TRY(rd->offsets.alloc((nkept + 2) * sizeof(uint64_t)));
  MG_TRY(rd->bases.alloc(rd->nbases + 16));
  hipLaunchKernelGGL(k_bam_seq_unpack, dim3(grid_for(nrec, kUnpackWaves, (unsigned)c.num_cus * 64)), dim3(64 * kUnpackWaves), 0, st,
                     d_bytes, d_off, nrec, d_keep, d_rank, d_pos, rd->bases.as<uint8_t>(), rd->offsets.as<uint64_t>());
  MG_HIP(hipGetLastError());
  *out = rd.release();
  return MG_OK;
}

// The header through zlib (gzread takes BGZF's members one after the other, and a plain file as it is).
int bam_read_header(const char* path, BamHeader* h) {
  gzFile g = gzopen(path, "rb");
  if (!g) return fail(MG_ERR_ARG, "cannot open %s", path);
  std::unique_ptr<gzFile_s, int (*)(gzFile)> guard(g, gzclose);
  auto rd = [&](void* dst, uint64_t len) -> bool {
    uint8_t* p = (uint8_t*)dst;
    while (len) {
      const unsigned step = len > (1u << 30) ? (1u << 30) : (unsigned)len;
      const int got = gzread(g, p, step);
      if (got <= 0) return false;
      p += got;
      len -= (uint64_t)got;
    }
    return true;
  };
  char magic[4];
  int32_t l_text = 0, n_ref = 0;
  if (!rd(magic, 4) || memcmp(magic, "BAM\1", 4) != 0) return fail(MG_ERR_ARG, "%s: not a BAM file (no BAM\\1 magic)", path);
  if (!rd(&l_text, 4) || l_text < 0) return fail(MG_ERR_ARG, "%s: truncated or corrupt BAM header", path);
  h->text.resize((size_t)l_text);
  if ((l_text && !rd(&h->text[0], (uint64_t)l_text)) || !rd(&n_ref, 4) || n_ref < 0)
    return fail(MG_ERR_ARG, "%s: truncated or corrupt BAM header", path);
  uint64_t bytes = 12ull + (uint64_t)l_text;
  h->names.clear();
  for (int32_t i = 0; i < n_ref; ++i) {
    int32_t l_name = 0, l_ref = 0;
    if (!rd(&l_name, 4) || l_name < 1) return fail(MG_ERR_ARG, "%s: truncated or corrupt BAM header", path);
    std::string nm((size_t)l_name, '\0');
    if (!rd(&nm[0], (uint64_t)l_name) || !rd(&l_ref, 4)) return fail(MG_ERR_ARG, "%s: truncated or corrupt BAM header", path);
    nm.resize(strnlen(nm.c_str(), (size_t)l_name));
    h->names.push_back(std::move(nm));
    bytes += 8ull + (uint64_t)l_name;
  }
  h->bytes = bytes;
  return MG_OK;
}

// refmap[0] = the row of '*' (refID -1), refmap[1 + i] = the row of reference i's name (-1: none; -2: not one SAM field)
std::vector<int32_t> bam_refmap(const std::vector<std::string>& names, const mg_acc_index* ix) {
  std::vector<int32_t> m(names.size() + 1, -1);
  auto row = [&](const std::string& s) -> int32_t {
    bool field = !s.empty();
    for (unsigned char ch : s) field = field && mgb::graph(ch);
    if (!field) return -2;
    auto it = ix->host_rows.find(s);
    return it == ix->host_rows.end() ? -1 : (int32_t)it->second;
  };
  m[0] = row("*");
  for (size_t i = 0; i < names.size(); ++i) m[i + 1] = row(names[i]);
  return m;
}

}  // namespace mg

using namespace mg;

extern "C" {

static int bam_tokenize_dev_impl(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* refmap, uint32_t nref, const mg_acc_index* ix,
                                const char* prev_qname, int final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec,
                                bool keyed, bool named = false, bool placed = false, bool edited = false, bool based = false) {
  MG_REQUIRE_READY();
  if (!out || !ix || (nref && !refmap) || nref > 0x7fffffffu) return fail(MG_ERR_ARG, "null argument");
  std::vector<int32_t> m(nref + 1ull);
  auto it = ix->host_rows.find("*");
  m[0] = it == ix->host_rows.end() ? -1 : (int32_t)it->second;
  for (uint32_t i = 0; i < nref; ++i) m[i + 1] = refmap[i] < -2 ? -1 : refmap[i];
  DevBuf d_map;
  MG_TRY(d_map.alloc(m.size() * sizeof(int32_t)));
  MG_TRY(mg_memcpy_h2d(d_map.p, m.data(), m.size() * sizeof(int32_t)));
  const int rc = bam_tokenize_prefix_dev(d_bytes, nbytes, d_map.as<int32_t>(), (int32_t)nref, prev_qname, final != 0, consumed, out,
                                         err_kind, err_rec, keyed, named, placed, edited, based);
  (void)hipStreamSynchronize(ctx().stream);  // (d_map is released here)
  return rc;
}

int mg_bam_tokenize_dev(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* refmap, uint32_t nref, const mg_acc_index* ix,
                        const char* prev_qname, int final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec) {
  return bam_tokenize_dev_impl(d_bytes, nbytes, refmap, nref, ix, prev_qname, final, consumed, out, err_kind, err_rec, false);
}

int mg_bam_tokenize_keyed_dev(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* refmap, uint32_t nref, const mg_acc_index* ix,
                              const char* prev_qname, int final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec) {
  return bam_tokenize_dev_impl(d_bytes, nbytes, refmap, nref, ix, prev_qname, final, consumed, out, err_kind, err_rec, true);
}

int mg_bam_tokenize_named_dev(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* refmap, uint32_t nref, const mg_acc_index* ix,
                              const char* prev_qname, int final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec) {
  return bam_tokenize_dev_impl(d_bytes, nbytes, refmap, nref, ix, prev_qname, final, consumed, out, err_kind, err_rec, false, true);
}

int mg_bam_tokenize_dev_ex(const uint8_t* d_bytes, uint64_t nbytes, const int32_t* refmap, uint32_t nref, const mg_acc_index* ix,
                           const char* prev_qname, int final, uint64_t* consumed, mg_sam_batch** out, int* err_kind, uint64_t* err_rec,
                           unsigned want) {
  if (want & ~(MG_BATCH_KEYS | MG_BATCH_NAMES | MG_BATCH_PLACES | MG_BATCH_COLLATE | MG_BATCH_EDITS | MG_BATCH_BASES)) return fail(MG_ERR_ARG, "unknown bits in want");
  if ((want & MG_BATCH_NAMES) && (want & MG_BATCH_COLLATE))
    return fail(MG_ERR_STATE, "a named batch is not collated (its names are in the order the reads came in)");
  const bool collate = (want & MG_BATCH_COLLATE) != 0;
  MG_TRY(bam_tokenize_dev_impl(d_bytes, nbytes, refmap, nref, ix, prev_qname, final, consumed, out, err_kind, err_rec,
                               collate || (want & MG_BATCH_KEYS), (want & MG_BATCH_NAMES) != 0, (want & MG_BATCH_PLACES) != 0,
                               (want & MG_BATCH_EDITS) != 0, (want & MG_BATCH_BASES) != 0));
  if (collate) {
    const int rc = collate_batch(*out, nullptr);
    if (rc != MG_OK) { delete *out; *out = nullptr; return rc; }
  }
  return MG_OK;
}

int mg_reads_parse_bam_prefix_dev(const uint8_t* d_bytes, uint64_t nbytes, int32_t n_ref, int final, uint64_t* consumed, mg_reads** out,
                                  uint64_t* err_at) {
  if (!consumed) return fail(MG_ERR_ARG, "null consumed");
  return bam_reads_prefix_dev(d_bytes, nbytes, n_ref, final != 0, consumed, out, err_at);
}

}  // extern "C"
