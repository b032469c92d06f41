// mg_genome.hip — organism FASTA files already in HBM -> one genome per FILE (`build_db --ingest device`; SURVEY.md §8 f2').
//
// The text of many files lies back to back in one buffer, file f = bytes [ext[f], ext[f + 1]).  Out come bases u8[] and
// offsets u64[nfiles + 1], one entry per file, as metalign_amd/build_db.py: genome_bases defines them (mg_genome_core.h holds the
// per-line rules, shared with the host check).  The flow:
//
//   k_gn_count / k_gn_mark   the positions of '\n', sixteen bytes per thread; the pass that reads every byte also looks for the
//                            bytes on which Python's text mode parts from these rules (an UNDECIDED file: the caller's)
//   k_gn_files               per file: its first '\n', and whether its last line lacks one (a VIRTUAL end: a file's last line
//                            never runs into the next file's first)
//   k_gn_lines               per line: its file, header or not, the stripped span
//   k_gn_emit                ... what it emits: nothing in front of the file's first header, 'N' for every later header, the
//                            stripped bytes of a sequence line — ranks are taken PER FILE
//   k_gn_offsets, k_gn_gather   the genomes' starts; the bytes, sixteen lanes per line and eight bytes per lane
//
// Lengths are per line (u32); positions and genome lengths are u64.
#include <memory>
#include <vector>

#include "mg_genome_core.h"
#include "mg_internal.h"

namespace mg {

constexpr int kGB = 256;   // threads per block
constexpr int kGW = 16;    // bytes per thread of the counting passes
constexpr int kGL = 16;    // lanes per line of the gather

// Thread g of the counting passes looks at the 16-byte ALIGNED window of memory number g counted from the aligned address at or
// below `text` (mg_ingest.hip: nl_window).
__device__ __forceinline__ int64_t gn_window(const uint8_t* text, uint64_t g) {
  return (int64_t)(g * kGW) - (int64_t)(reinterpret_cast<uintptr_t>(text) & 15);
}

// file of byte o: the last f with ext[f] <= o (empty files share their start with the next one, which is the one taken)
__device__ __forceinline__ uint64_t gn_file_of(const uint64_t* __restrict__ ext, uint64_t nfiles, uint64_t o) {
  uint64_t lo = 0, hi = nfiles;  // ext[lo] <= o < ext[hi]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (ext[mid] <= o) lo = mid; else hi = mid;
  }
  return lo;
}

// bit j set <=> text[base + j] == '\n' (offsets outside [0, nbytes) never).  A window with a byte that MAY leave its file
// undecided (>= 0x80, 0x1c-0x1f, '\r') is looked at byte by byte; a '\r' is taken with the byte behind it in the BUFFER — the
// one '\r' this lets through, a file's last byte in front of a file that begins with '\n', ends a line without '\n' and is
// k_gn_lines'.
__device__ __forceinline__ uint32_t gn_mask16(const uint8_t* __restrict__ text, uint64_t nbytes, int64_t base,
                                              const uint64_t* __restrict__ ext, uint64_t nfiles, uint32_t* __restrict__ und) {
  uint32_t m = 0;
  bool slow = true;
  if (base >= 0 && (uint64_t)base + kGW <= nbytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t sus = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int b = 0; b < 4; ++b) m |= (((w[q] >> (8 * b)) & 0xffu) == 0x0au ? 1u : 0u) << (4 * q + b);
      const uint32_t c = (w[q] ^ 0x1c1c1c1cu) & 0xfcfcfcfcu, r = w[q] ^ 0x0d0d0d0du;  // a zero byte: 0x1c-0x1f / '\r'
      sus |= (w[q] | ((c - 0x01010101u) & ~c) | ((r - 0x01010101u) & ~r)) & 0x80808080u;
    }
    slow = sus != 0;
    if (!slow) return m;
    m = 0;
  }
  for (int j = 0; j < kGW; ++j) {
    const int64_t o = base + j;
    if (o < 0 || (uint64_t)o >= nbytes) continue;
    const uint8_t ch = text[o];
    if (ch == '\n') m |= 1u << j;
    const bool has_next = (uint64_t)o + 1 < nbytes;
    if (mgg::undecided_byte(ch, has_next, has_next ? text[o + 1] : 0)) und[gn_file_of(ext, nfiles, (uint64_t)o)] = 1u;
  }
  return m;
}

__global__ __launch_bounds__(kGB) void k_gn_count(const uint8_t* __restrict__ text, uint64_t nbytes, const uint64_t* __restrict__ ext,
                                                  uint64_t nfiles, uint32_t* __restrict__ und, uint32_t* __restrict__ blk_count) {
  __shared__ uint32_t wsum[kGB / 64];
  const int64_t base = gn_window(text, (uint64_t)blockIdx.x * kGB + threadIdx.x);
  uint32_t c = base < (int64_t)nbytes ? __popc(gn_mask16(text, nbytes, base, ext, nfiles, und)) : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// line_end[i] = byte offset of the i-th '\n'
__global__ __launch_bounds__(kGB) void k_gn_mark(const uint8_t* __restrict__ text, uint64_t nbytes, const uint64_t* __restrict__ blk_base,
                                                 uint64_t* __restrict__ line_end) {
  __shared__ uint32_t wsum[kGB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = gn_window(text, (uint64_t)blockIdx.x * kGB + threadIdx.x);
  uint32_t m = 0;
  if (base >= 0 && (uint64_t)base + kGW <= nbytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < 4; ++b) m |= (((w[q] >> (8 * b)) & 0xffu) == 0x0au ? 1u : 0u) << (4 * q + b);
  } else if (base < (int64_t)nbytes) {
    for (int j = 0; j < kGW; ++j) {
      const int64_t o = base + j;
      if (o >= 0 && (uint64_t)o < nbytes && text[o] == '\n') m |= 1u << j;
    }
  }
  const uint32_t c = __popc(m);
  uint32_t inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t p = __shfl_up(inc, o, 64);
    if (lane >= o) inc += p;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wsum[w];
  uint64_t at = blk_base[blockIdx.x] + before + inc - c;
  while (m) {
    const int j = __ffs(m) - 1;
    line_end[at++] = (uint64_t)(base + j);
    m &= m - 1;
  }
}

// first_nl[f] = the number of '\n' in front of file f (f <= nfiles); virt[f] = file f's last line ends without one
__global__ void k_gn_files(const uint8_t* __restrict__ text, const uint64_t* __restrict__ ext, uint64_t nfiles,
                           const uint64_t* __restrict__ line_end, uint64_t nnl, uint64_t* __restrict__ first_nl,
                           uint32_t* __restrict__ virt) {
  uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; f <= nfiles; f += stride) {
    const uint64_t at = ext[f];
    uint64_t lo = 0, hi = nnl;  // the first i with line_end[i] >= at
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (line_end[mid] < at) lo = mid + 1; else hi = mid;
    }
    first_nl[f] = lo;
    virt[f] = f < nfiles && ext[f + 1] > at && text[ext[f + 1] - 1] != '\n' ? 1u : 0u;
  }
}

// line_base[f] = the number of lines in front of file f: the '\n' and the virtual ends
__global__ void k_gn_line_base(const uint64_t* __restrict__ first_nl, const uint64_t* __restrict__ virt_before, uint64_t nfiles,
                               uint64_t* __restrict__ line_base) {
  uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; f <= nfiles; f += stride) line_base[f] = first_nl[f] + virt_before[f];
}

// Line l: its file, header or not, the start and the length of its stripped span.  A line that ends in '\r' without a '\n'
// behind it leaves its file undecided (the one case k_gn_count cannot see), and so does a header without a name.
__global__ void k_gn_lines(const uint8_t* __restrict__ text, const uint64_t* __restrict__ ext, uint64_t nfiles,
                           const uint64_t* __restrict__ line_end, const uint64_t* __restrict__ first_nl,
                           const uint64_t* __restrict__ line_base, uint64_t nlines, uint32_t* __restrict__ lfile,
                           uint32_t* __restrict__ flags, uint32_t* __restrict__ lens, uint64_t* __restrict__ sbeg,
                           uint32_t* __restrict__ und) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; l < nlines; l += stride) {
    const uint64_t f = gn_file_of(line_base, nfiles, l);  // (a file without lines shares its base with the next one)
    const uint64_t j = l - line_base[f], nl0 = first_nl[f], nnl = first_nl[f + 1] - nl0;
    const uint64_t beg = j == 0 ? ext[f] : line_end[nl0 + j - 1] + 1;
    const bool virt = j >= nnl;
    const uint64_t end = virt ? ext[f + 1] : line_end[nl0 + j];
    if (virt && end > beg && text[end - 1] == '\r') und[f] = 1u;
    uint64_t sb, se;
    const bool head = mgg::classify_line(text, beg, end, &sb, &se);
    if (mgg::nameless_header(head, se - sb, end - beg, !virt)) und[f] = 1u;
    lfile[l] = (uint32_t)f;
    flags[l] = head ? 1u : 0u;
    lens[l] = (uint32_t)(se - sb);
    sbeg[l] = sb;
  }
}

// lens[l]: the stripped length -> what the line emits (rank: the headers in front of the line, of every file)
__global__ void k_gn_emit(const uint32_t* __restrict__ lfile, const uint32_t* __restrict__ flags, const uint64_t* __restrict__ rank,
                          const uint64_t* __restrict__ line_base, uint64_t nlines, uint32_t* __restrict__ lens) {
  uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; l < nlines; l += stride) lens[l] = mgg::emitted(flags[l] != 0, lens[l], rank[l] - rank[line_base[lfile[l]]]);
}

__global__ void k_gn_offsets(const uint64_t* __restrict__ line_base, const uint64_t* __restrict__ pos, uint64_t nfiles,
                             uint64_t nlines, uint64_t nbases, uint64_t* __restrict__ offsets) {
  uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; f <= nfiles; f += stride) offsets[f] = line_base[f] < nlines ? pos[line_base[f]] : nbases;
}

// Sixteen lanes per line.  A genome line is 60-80 bytes at any address on either side: the destination is written in aligned
// 8-byte words, each assembled from the two aligned source words it straddles (every word loaded holds a byte of the span), the
// bytes in front of the first and behind the last whole word singly.
__global__ __launch_bounds__(kGB) void k_gn_gather(const uint8_t* __restrict__ text, const uint32_t* __restrict__ flags,
                                                   const uint32_t* __restrict__ lens, const uint64_t* __restrict__ sbeg,
                                                   const uint64_t* __restrict__ pos, uint64_t nlines, uint8_t* __restrict__ bases) {
  const uint32_t sub = threadIdx.x & (kGL - 1);
  uint64_t l = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGL;
  const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / kGL;
  for (; l < nlines; l += stride) {
    const uint32_t n = lens[l];
    if (!n) continue;
    uint8_t* dst = bases + pos[l];
    if (flags[l]) {
      if (sub == 0) dst[0] = 'N';
      continue;
    }
    const uint8_t* src = text + sbeg[l];
    uint32_t head = (uint32_t)((8u - (reinterpret_cast<uintptr_t>(dst) & 7u)) & 7u);
    if (head > n) head = n;
    if (sub < head) dst[sub] = src[sub];
    const uint32_t nw = (n - head) >> 3;
    for (uint32_t w = sub; w < nw; w += kGL) {
      const uint8_t* s = src + head + 8u * w;
      const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 7u);
      const uint64_t* a = reinterpret_cast<const uint64_t*>(s - sh);
      uint64_t v = a[0];
      if (sh) v = (v >> (8u * sh)) | (a[1] << (64u - 8u * sh));
      *reinterpret_cast<uint64_t*>(dst + head + 8u * w) = v;
    }
    const uint32_t done = head + 8u * nw;
    if (sub < n - done) dst[done + sub] = src[done + sub];
  }
}

}  // namespace mg

using namespace mg;

extern "C" {

int mg_genomes_parse_dev(const uint8_t* d_text, const uint64_t* file_extents, uint64_t nfiles, mg_genomes** out, uint8_t* undecided) {
  MG_REQUIRE_READY();
  if (!out) return fail(MG_ERR_ARG, "null out handle");
  *out = nullptr;
  if (nfiles && !file_extents) return fail(MG_ERR_ARG, "null file extents");
  if (nfiles >= 0xffffffffull) return fail(MG_ERR_ARG, "too many files for one batch");
  for (uint64_t f = 0; f < nfiles; ++f)
    if (file_extents[f + 1] < file_extents[f]) return fail(MG_ERR_ARG, "file extents must ascend");
  Context& c = ctx();
  hipStream_t st = c.stream;
  std::unique_ptr<mg_genomes> gn(new mg_genomes());
  gn->ngenomes = nfiles;
  gn->h_offsets.assign(nfiles + 1, 0);
  const uint64_t t0 = nfiles ? file_extents[0] : 0;
  const uint64_t nbytes = nfiles ? file_extents[nfiles] - t0 : 0;
  if (nbytes && !d_text) return fail(MG_ERR_ARG, "null device text");
  const uint8_t* text = d_text + t0;
  std::vector<uint64_t> rel(nfiles + 1, 0);
  for (uint64_t f = 0; f <= nfiles && nfiles; ++f) rel[f] = file_extents[f] - t0;
  MG_TRY(gn->offsets.alloc((nfiles + 2) * sizeof(uint64_t)));
  const bool guard = dbg("genome_guard") != 0;
  auto finish_empty = [&]() -> int {
    MG_TRY(gn->bases.alloc(16));
    MG_HIP(hipMemsetAsync(gn->offsets.p, 0, (nfiles + 1) * sizeof(uint64_t), st));
    if (guard) {
      MG_HIP(hipMemsetAsync(gn->bases.p, 0xa5, 16, st));
      MG_HIP(hipMemsetAsync(gn->offsets.as<uint64_t>() + nfiles + 1, 0xa5, sizeof(uint64_t), st));
    }
    MG_HIP(hipStreamSynchronize(st));
    if (undecided) for (uint64_t f = 0; f < nfiles; ++f) undecided[f] = 0;
    *out = gn.release();
    return MG_OK;
  };
  if (nbytes == 0) return finish_empty();

  ProfScope ps("ingest_genomes");
  const uint64_t per_block = (uint64_t)kGB * kGW;
  const uint64_t nblocks = (nbytes + (kGW - 1) + per_block - 1) / per_block;  // (up to 15 bytes of slack in front of the text)
  if (nblocks > 0x7fffffffull) return fail(MG_ERR_ARG, "text too large for one ingest call");
  uint64_t* d_ext = (uint64_t*)scratch("gn_ext", (nfiles + 1) * sizeof(uint64_t));
  uint32_t* d_und = (uint32_t*)scratch("gn_und", nfiles * sizeof(uint32_t));
  uint32_t* d_cnt = (uint32_t*)scratch("gn_blk_cnt", nblocks * sizeof(uint32_t));
  uint64_t* d_base = (uint64_t*)scratch("gn_blk_base", (nblocks + 1) * sizeof(uint64_t));
  uint64_t* d_first = (uint64_t*)scratch("gn_first_nl", (nfiles + 1) * sizeof(uint64_t));
  uint32_t* d_virt = (uint32_t*)scratch("gn_virt", (nfiles + 1) * sizeof(uint32_t));
  uint64_t* d_vbefore = (uint64_t*)scratch("gn_virt_before", (nfiles + 1) * sizeof(uint64_t));
  uint64_t* d_lbase = (uint64_t*)scratch("gn_line_base", (nfiles + 1) * sizeof(uint64_t));
  if (!d_ext || !d_und || !d_cnt || !d_base || !d_first || !d_virt || !d_vbefore || !d_lbase) return MG_ERR_NOMEM;
  MG_HIP(hipMemcpyAsync(d_ext, rel.data(), (nfiles + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MG_HIP(hipMemsetAsync(d_und, 0, nfiles * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_gn_count, dim3((unsigned)nblocks), dim3(kGB), 0, st, text, nbytes, d_ext, nfiles, d_und, d_cnt);
  MG_HIP(hipGetLastError());
  uint64_t nnl = 0, nvirt = 0;
  MG_TRY(exclusive_sum_u32_to_u64(d_cnt, d_base, nblocks, &nnl));  // (synchronises: rel may go after it)
  uint64_t* d_le = (uint64_t*)scratch("gn_lines", (nnl + 2) * sizeof(uint64_t));
  if (!d_le) return MG_ERR_NOMEM;
  hipLaunchKernelGGL(k_gn_mark, dim3((unsigned)nblocks), dim3(kGB), 0, st, text, nbytes, d_base, d_le);
  const unsigned fgrid = grid_for(nfiles + 1, 256, (unsigned)c.num_cus * 8);
  hipLaunchKernelGGL(k_gn_files, dim3(fgrid), dim3(256), 0, st, text, d_ext, nfiles, d_le, nnl, d_first, d_virt);
  MG_HIP(hipGetLastError());
  // (nfiles inputs -> nfiles + 1 outputs, the last the total: what d_vbefore holds; virt[nfiles] is 0 and needs no place in the sum)
  MG_TRY(exclusive_sum_u32_to_u64(d_virt, d_vbefore, nfiles, &nvirt));
  hipLaunchKernelGGL(k_gn_line_base, dim3(fgrid), dim3(256), 0, st, d_first, d_vbefore, nfiles, d_lbase);
  MG_HIP(hipGetLastError());
  const uint64_t nlines = nnl + nvirt;  // > 0: the text is not empty
  uint32_t* d_lfile = (uint32_t*)scratch("gn_lfile", nlines * sizeof(uint32_t));
  uint32_t* d_flag = (uint32_t*)scratch("gn_flag", nlines * sizeof(uint32_t));
  uint32_t* d_len = (uint32_t*)scratch("gn_len", nlines * sizeof(uint32_t));
  uint64_t* d_sbeg = (uint64_t*)scratch("gn_sbeg", nlines * sizeof(uint64_t));
  uint64_t* d_rank = (uint64_t*)scratch("gn_rank", (nlines + 1) * sizeof(uint64_t));
  uint64_t* d_pos = (uint64_t*)scratch("gn_pos", (nlines + 1) * sizeof(uint64_t));
  if (!d_lfile || !d_flag || !d_len || !d_sbeg || !d_rank || !d_pos) return MG_ERR_NOMEM;
  const unsigned lgrid = grid_for(nlines, 256, (unsigned)c.num_cus * 8);
  hipLaunchKernelGGL(k_gn_lines, dim3(lgrid), dim3(256), 0, st, text, d_ext, nfiles, d_le, d_first, d_lbase, nlines, d_lfile, d_flag,
                     d_len, d_sbeg, d_und);
  MG_HIP(hipGetLastError());
  uint64_t nhead = 0, nbases = 0;
  MG_TRY(exclusive_sum_u32_to_u64(d_flag, d_rank, nlines, &nhead));
  hipLaunchKernelGGL(k_gn_emit, dim3(lgrid), dim3(256), 0, st, d_lfile, d_flag, d_rank, d_lbase, nlines, d_len);
  MG_HIP(hipGetLastError());
  MG_TRY(exclusive_sum_u32_to_u64(d_len, d_pos, nlines, &nbases));
  gn->nbases = nbases;
  MG_TRY(gn->bases.alloc(nbases + 16));
  if (guard) {
    MG_HIP(hipMemsetAsync(gn->bases.as<uint8_t>() + nbases, 0xa5, 16, st));
    MG_HIP(hipMemsetAsync(gn->offsets.as<uint64_t>() + nfiles + 1, 0xa5, sizeof(uint64_t), st));
  }
  hipLaunchKernelGGL(k_gn_offsets, dim3(fgrid), dim3(256), 0, st, d_lbase, d_pos, nfiles, nlines, nbases, gn->offsets.as<uint64_t>());
  hipLaunchKernelGGL(k_gn_gather, dim3(grid_for(nlines, kGB / kGL, (unsigned)c.num_cus * 16)), dim3(kGB), 0, st, text, d_flag, d_len,
                     d_sbeg, d_pos, nlines, gn->bases.as<uint8_t>());
  MG_HIP(hipGetLastError());
  std::vector<uint32_t> h_und(nfiles);
  MG_HIP(hipMemcpyAsync(gn->h_offsets.data(), gn->offsets.p, (nfiles + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipMemcpyAsync(h_und.data(), d_und, nfiles * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MG_HIP(hipStreamSynchronize(st));
  // (a file of 2^32 bytes or more may hold a line whose length no u32 holds: the caller's, like the undecided bytes)
  if (undecided) for (uint64_t f = 0; f < nfiles; ++f) undecided[f] = h_und[f] || rel[f + 1] - rel[f] > 0xffffffffull ? 1 : 0;
  *out = gn.release();
  return MG_OK;
}

uint64_t mg_genomes_count(const mg_genomes* g) { return g ? g->ngenomes : 0; }
uint64_t mg_genomes_nbases(const mg_genomes* g) { return g ? g->nbases : 0; }

int mg_genomes_device_ptrs(const mg_genomes* g, const uint8_t** d_bases, const uint64_t** d_offsets) {
  if (!g) return fail(MG_ERR_ARG, "null genomes");
  if (d_bases) *d_bases = g->bases.as<uint8_t>();
  if (d_offsets) *d_offsets = g->offsets.as<uint64_t>();
  return MG_OK;
}

int mg_genomes_download(const mg_genomes* g, uint8_t* bases, uint64_t* offsets) {
  MG_REQUIRE_READY();
  if (!g) return fail(MG_ERR_ARG, "null genomes");
  if (bases && g->nbases) MG_TRY(mg_memcpy_d2h(bases, g->bases.p, g->nbases));
  if (offsets) MG_TRY(mg_memcpy_d2h(offsets, g->offsets.p, (g->ngenomes + 1) * sizeof(uint64_t)));
  return MG_OK;
}

void mg_genomes_free(mg_genomes* g) { delete g; }

}  // extern "C"
