// mg_refseq.hip — the reference FASTA, already in HBM, parsed BY RECORD into one code byte per site of the accession rows (--ani,
// --vcf; metalign_amd/refseq.py is the definition, mg_refseq_core.h holds the per-byte, per-line and per-record rules, shared with
// the host check).  mg_genome.hip makes one genome per FILE and throws the names away; here every record is resolved to its
// accession row and lands at the site offset mg_variants_create derives from the same lengths.  The flow:
//
//   build_line_index   the positions of '\n', sixteen bytes per thread: the tokenisers' own (mg_ingest.hip)
//   k_rs_lines         per line: header or not; a sequence line's stripped span, a header's name start
//   (two scans)        rank[l] = the headers in front of line l: a sequence line belongs to record rank[l] - 1, none in front of the
//                      first header; pos[l] = the bases in front of line l, so a line's base rank inside its record is
//                      pos[l] - pos[its record's header line]
//   k_rs_records       per header line: the record's line and its accession row (mg_acc_dev.h: acc_lookup, the look-up the SAM
//                      tokeniser resolves RNAME with); the FIRST record of every row by a 64-bit atomic minimum over record
//                      numbers, so "the first record wins" holds whatever the grid
//   k_rs_kinds         per record: its bases, its kind (mgrs::kind_of), where its codes go; the five counters
//   k_rs_gather        the codes of the loaded records, sixteen lanes per line and eight bytes per lane
//
// A row that is not loaded is never written: its bytes keep the 0xff the array is created with, and mg_variants_diff never reads
// them.  Lengths are per line (u32); positions, record numbers and site offsets are u64.
#include <memory>
#include <vector>

#include "mg_acc_dev.h"
#include "mg_internal.h"
#include "mg_refseq_core.h"

using namespace mg;

namespace {

constexpr int kRB = 256;  // threads per block
constexpr int kRL = 16;   // lanes per line of the gather
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr uint64_t kNoDst = ~0ull;

__device__ __forceinline__ uint64_t rs_line_beg(const uint64_t* __restrict__ line_end, uint64_t l) { return l ? line_end[l - 1] + 1 : 0; }

// flags[l] = header; lens[l] = the bases a sequence line carries (a header: 0); sbeg[l] = where they, or the header's name, start
__global__ __launch_bounds__(kRB) void k_rs_lines(const uint8_t* __restrict__ text, const uint64_t* __restrict__ line_end, uint64_t nlines,
                                                  uint32_t* __restrict__ flags, uint32_t* __restrict__ lens, uint64_t* __restrict__ sbeg,
                                                  uint32_t* __restrict__ too_long) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; l < nlines; l += stride) {
    const mgrs::Line ln = mgrs::classify_line(text, rs_line_beg(line_end, l), line_end[l]);
    uint64_t n = ln.head ? 0 : ln.e - ln.b;
    if (n > 0xffffffffull) {
      *too_long = 1u;
      n = 0;
    }
    flags[l] = ln.head ? 1u : 0u;
    lens[l] = (uint32_t)n;
    sbeg[l] = ln.b;
  }
}

// Header line l opens record rank[l]: its line, its row (kNoRow: foreign) and the row's first record.
__global__ __launch_bounds__(kRB) void k_rs_records(const uint8_t* __restrict__ text, const uint64_t* __restrict__ line_end,
                                                    const uint32_t* __restrict__ flags, const uint64_t* __restrict__ rank,
                                                    const uint64_t* __restrict__ sbeg, uint64_t nlines, AccTable acc,
                                                    uint64_t* __restrict__ rec_line, uint32_t* __restrict__ rec_row,
                                                    unsigned long long* __restrict__ first) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; l < nlines; l += stride) {
    if (!flags[l]) continue;
    const uint64_t r = rank[l], b = sbeg[l], end = line_end[l];
    uint64_t e = b;  // (the name again: mgrs::classify_line's rule for a header)
    while (e < end && !mgrs::is_white(text[e])) ++e;
    const int64_t row = e > b && e - b <= 0xffffffffull ? acc_lookup(acc, text + b, (uint32_t)(e - b)) : -1;
    rec_line[r] = l;
    rec_row[r] = row < 0 ? kNoRow : (uint32_t)row;
    if (row >= 0) atomicMin(&first[row], (unsigned long long)r);
  }
}

// Record r: its bases are those between its header line and the next one (pos of a header = the bases in front of it).
// stats4: loaded, foreign, mismatched, duplicate.
__global__ __launch_bounds__(kRB) void k_rs_kinds(const uint64_t* __restrict__ rec_line, const uint32_t* __restrict__ rec_row,
                                                  const unsigned long long* __restrict__ first, const uint64_t* __restrict__ pos,
                                                  uint64_t nrec, uint64_t nbases, const uint64_t* __restrict__ len,
                                                  const uint64_t* __restrict__ off, uint64_t* __restrict__ rec_dst,
                                                  uint8_t* __restrict__ loaded, unsigned long long* __restrict__ stats4) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  // (uniform trip count: every lane takes part in the ballots)
  for (uint64_t r0 = (uint64_t)blockIdx.x * blockDim.x; r0 < nrec; r0 += stride) {
    const uint64_t r = r0 + threadIdx.x;
    uint32_t kind = 4;  // (no record)
    if (r < nrec) {
      const uint64_t nb = (r + 1 < nrec ? pos[rec_line[r + 1]] : nbases) - pos[rec_line[r]];
      const uint32_t row = rec_row[r];
      const bool has_row = row != kNoRow;
      kind = mgrs::kind_of(has_row, has_row && first[row] == r, nb, has_row ? len[row] : 0);
      rec_dst[r] = kind == mgrs::kLoaded ? off[row] : kNoDst;
      if (kind == mgrs::kLoaded) loaded[row] = 1;
    }
    for (uint32_t k = 0; k < 4; ++k) {
      const unsigned long long m = __ballot(kind == k);
      if (m && (threadIdx.x & 63u) == 0) atomicAdd(&stats4[k], (unsigned long long)__builtin_popcountll(m));
    }
  }
}

__device__ __forceinline__ uint64_t rs_codes8(uint64_t v) {
  uint64_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= (uint64_t)mgvar::code_of((uint32_t)(v >> (8 * i)) & 0xffu) << (8 * i);
  return o;
}

// Sixteen lanes per line, as k_gn_gather (mg_genome.hip): the destination is written in aligned 8-byte words, each assembled from
// the two aligned source words it straddles (every word loaded holds a byte of the span), the bytes in front of the first and
// behind the last whole word singly — every byte through code_of on its way.  A loaded record has exactly its row's length in
// bases, so every byte written lies inside the row.
__global__ __launch_bounds__(kRB) void k_rs_gather(const uint8_t* __restrict__ text, const uint32_t* __restrict__ flags,
                                                   const uint32_t* __restrict__ lens, const uint64_t* __restrict__ sbeg,
                                                   const uint64_t* __restrict__ pos, const uint64_t* __restrict__ rank,
                                                   const uint64_t* __restrict__ rec_line, const uint64_t* __restrict__ rec_dst,
                                                   uint64_t nlines, uint8_t* __restrict__ codes) {
  const uint32_t sub = threadIdx.x & (kRL - 1);
  uint64_t l = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kRL;
  const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / kRL;
  for (; l < nlines; l += stride) {
    const uint32_t n = lens[l];
    if (!n || flags[l]) continue;
    const uint64_t rk = rank[l];
    if (rk == 0) continue;  // (in front of the first header)
    const uint64_t at = rec_dst[rk - 1];
    if (at == kNoDst) continue;
    uint8_t* dst = codes + at + (pos[l] - pos[rec_line[rk - 1]]);
    const uint8_t* src = text + sbeg[l];
    uint32_t head = (uint32_t)((8u - (reinterpret_cast<uintptr_t>(dst) & 7u)) & 7u);
    if (head > n) head = n;
    if (sub < head) dst[sub] = (uint8_t)mgvar::code_of(src[sub]);
    const uint32_t nw = (n - head) >> 3;
    for (uint32_t w = sub; w < nw; w += kRL) {
      const uint8_t* s = src + head + 8u * w;
      const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 7u);
      const uint64_t* a = reinterpret_cast<const uint64_t*>(s - sh);
      uint64_t v = a[0];
      if (sh) v = (v >> (8u * sh)) | (a[1] << (64u - 8u * sh));
      *reinterpret_cast<uint64_t*>(dst + head + 8u * w) = rs_codes8(v);
    }
    const uint32_t done = head + 8u * nw;
    if (sub < n - done) dst[done + sub] = (uint8_t)mgvar::code_of(src[done + sub]);
  }
}

}  // namespace

extern "C" {

int mg_refseq_parse_dev(const uint8_t* d_text, uint64_t nbytes, const mg_acc_index* ix, const uint64_t* lengths, uint32_t nacc,
                        mg_refseq** out) {
  MG_REQUIRE_READY();
  if (!out || !ix || (nacc && !lengths) || (nbytes && !d_text)) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  if (ix->nacc != nacc) return fail(MG_ERR_ARG, "the accession index has %u rows, the lengths %u", ix->nacc, nacc);
  Context& c = ctx();
  hipStream_t st = c.stream;
  std::unique_ptr<mg_refseq> h(new mg_refseq());
  h->nacc = nacc;
  std::vector<uint64_t> h_off(nacc + 1ull, 0);
  for (uint32_t a = 0; a < nacc; ++a) {
    if (lengths[a] >> 48) return fail(MG_ERR_ARG, "accession %u: length %llu", a, (unsigned long long)lengths[a]);
    h_off[a + 1] = h_off[a] + lengths[a];
  }
  h->nsites = h_off[nacc];
  h->h_len.assign(lengths, lengths + nacc);
  const uint64_t bytes = h->nsites + 16;
  MG_TRY(own_alloc((void**)&h->codes, bytes, "the reference codes (%llu bytes, one per reference base) do not fit: %s", bytes));
  MG_TRY(h->loaded.alloc(nacc + 16ull));
  MG_HIP(hipMemsetAsync(h->codes, 0xff, bytes, st));
  MG_HIP(hipMemsetAsync(h->loaded.p, 0, nacc + 16ull, st));
  MG_HIP(hipStreamSynchronize(st));
  if (nbytes == 0) {
    *out = h.release();
    return MG_OK;
  }
  uint64_t* d_le = nullptr;
  uint64_t nlines = 0;
  bool vlast = false;
  MG_TRY(build_line_index(d_text, nbytes, &d_le, &nlines, &vlast));  // (> 0 lines: the text is not empty)

  ProfScope ps("refseq_parse");
  DevBuf flags, lens, sbeg, rank, pos, meta, small;
  const uint64_t line_bytes = nlines * 32 + 64;
  if (flags.alloc(nlines * sizeof(uint32_t)) != MG_OK || lens.alloc(nlines * sizeof(uint32_t)) != MG_OK ||
      sbeg.alloc(nlines * sizeof(uint64_t)) != MG_OK || rank.alloc((nlines + 1) * sizeof(uint64_t)) != MG_OK ||
      pos.alloc((nlines + 1) * sizeof(uint64_t)) != MG_OK)
    return fail(MG_ERR_NOMEM, "the line index of the reference (%llu bytes for %llu lines) does not fit on the device",
                (unsigned long long)line_bytes, (unsigned long long)nlines);
  // meta: the lengths u64[nacc], the offsets u64[nacc + 1], the rows' first records u64[nacc]; small: too_long u32 (+ pad), stats u64[4]
  MG_TRY(meta.alloc((3ull * nacc + 2) * sizeof(uint64_t)));
  MG_TRY(small.alloc(8 + 4 * sizeof(uint64_t)));
  uint64_t* d_len = meta.as<uint64_t>();
  uint64_t* d_off = d_len + nacc;
  unsigned long long* d_first = reinterpret_cast<unsigned long long*>(d_off + nacc + 1);
  uint32_t* d_long = small.as<uint32_t>();
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(small.as<uint8_t>() + 8);
  if (nacc) MG_HIP(hipMemcpyAsync(d_len, lengths, (uint64_t)nacc * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipMemcpyAsync(d_off, h_off.data(), (nacc + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipMemsetAsync(d_first, 0xff, (nacc + 1ull) * sizeof(uint64_t), st));
  MG_HIP(hipMemsetAsync(small.p, 0, 8 + 4 * sizeof(uint64_t), st));
  const unsigned lgrid = grid_for(nlines, kRB, (unsigned)c.num_cus * 8);
  hipLaunchKernelGGL(k_rs_lines, dim3(lgrid), dim3(kRB), 0, st, d_text, d_le, nlines, flags.as<uint32_t>(), lens.as<uint32_t>(),
                     sbeg.as<uint64_t>(), d_long);
  MG_HIP(hipGetLastError());
  uint64_t nrec = 0, nbases = 0;
  MG_TRY(exclusive_sum_u32_to_u64(flags.as<uint32_t>(), rank.as<uint64_t>(), nlines, &nrec));  // (synchronises: h_off may go)
  MG_TRY(exclusive_sum_u32_to_u64(lens.as<uint32_t>(), pos.as<uint64_t>(), nlines, &nbases));
  uint32_t too_long = 0;
  MG_HIP(hipMemcpyAsync(&too_long, d_long, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));
  if (too_long) return fail(MG_ERR_ARG, "the reference holds a line of 2^32 bases or more");
  h->stats[0] = nrec;
  if (nrec) {
    DevBuf rec_line, rec_row, rec_dst;
    if (rec_line.alloc(nrec * sizeof(uint64_t)) != MG_OK || rec_row.alloc(nrec * sizeof(uint32_t)) != MG_OK ||
        rec_dst.alloc(nrec * sizeof(uint64_t)) != MG_OK)
      return fail(MG_ERR_NOMEM, "the records of the reference (%llu bytes for %llu records) do not fit on the device",
                  (unsigned long long)(nrec * 20), (unsigned long long)nrec);
    hipLaunchKernelGGL(k_rs_records, dim3(lgrid), dim3(kRB), 0, st, d_text, d_le, flags.as<uint32_t>(), rank.as<uint64_t>(),
                       sbeg.as<uint64_t>(), nlines, acc_table_of(ix), rec_line.as<uint64_t>(), rec_row.as<uint32_t>(), d_first);
    MG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rs_kinds, dim3(grid_for(nrec, kRB, (unsigned)c.num_cus * 8)), dim3(kRB), 0, st, rec_line.as<uint64_t>(),
                       rec_row.as<uint32_t>(), d_first, pos.as<uint64_t>(), nrec, nbases, d_len, d_off, rec_dst.as<uint64_t>(),
                       h->loaded.as<uint8_t>(), d_stats);
    MG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rs_gather, dim3(grid_for(nlines, kRB / kRL, (unsigned)c.num_cus * 16)), dim3(kRB), 0, st, d_text,
                       flags.as<uint32_t>(), lens.as<uint32_t>(), sbeg.as<uint64_t>(), pos.as<uint64_t>(), rank.as<uint64_t>(),
                       rec_line.as<uint64_t>(), rec_dst.as<uint64_t>(), nlines, h->codes);
    MG_HIP(hipGetLastError());
    MG_HIP(hipMemcpyAsync(h->stats + 1, d_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MG_HIP(hipStreamSynchronize(st));  // (the record arrays go back to the pool behind their kernels)
  }
  *out = h.release();
  return MG_OK;
}

int mg_refseq_stats(const mg_refseq* h, uint64_t out5[5]) {
  if (!h || !out5) return fail(MG_ERR_ARG, "null argument");
  for (int i = 0; i < 5; ++i) out5[i] = h->stats[i];
  return MG_OK;
}

int mg_refseq_loaded(const mg_refseq* h, uint8_t* loaded) {
  MG_REQUIRE_READY();
  if (!h || (h->nacc && !loaded)) return fail(MG_ERR_ARG, "null argument");
  if (h->nacc) MG_TRY(mg_memcpy_d2h(loaded, h->loaded.p, h->nacc));
  return MG_OK;
}

int mg_refseq_download(const mg_refseq* h, uint8_t* codes) {
  MG_REQUIRE_READY();
  if (!h || (h->nsites && !codes)) return fail(MG_ERR_ARG, "null argument");
  if (h->nsites) MG_TRY(mg_memcpy_d2h(codes, h->codes, h->nsites));
  return MG_OK;
}

void mg_refseq_free(mg_refseq* h) { delete h; }

}  // extern "C"
