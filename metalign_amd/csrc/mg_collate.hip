// mg_collate.hip — alignment records regrouped by read on the device: what lets stage C take a coordinate-sorted SAM / BAM file.
//
// The reference closes a read when the QNAME changes (scripts/map_and_profile.py:220): all alignments of a read are expected
// next to each other, which `samtools sort` (by coordinate, its default) undoes.  metalign_amd/collate.py (collated_lines) is
// the DEFINITION of the regrouped order: the reads in the order of their first retained line, inside a read (mate-2 class, not
// primary, file index).  Here that is a permutation of ONE batch of 16-byte records plus a recomputed new-read bit:
//
//   keyed emit       (mg_ingest.hip: k_sam_emit<true>)  a 128-bit key per retained record, mg_collate_core.h: qname_key
//   sort by key      two stable 64-bit radix passes (hi, then lo) carrying the record index: equal names become runs, the
//                    indices ascending inside a run
//   k_collate_heads  a run begins where either half of the key changes; the head's POSITION, 0 elsewhere -> an inclusive
//   + max-scan       max-scan gives every record its run's head, whose index is the read's first appearance: the group id
//   k_collate_fkey   the final key  gid << 2 | mate2 << 1 | notprimary
//   sort by it       stable, so the file index breaks ties (ascending inside a run after the first sort)
//   k_collate_gather records through the permutation; bit 31 set on record 0 and wherever the group id changes, cleared elsewhere
//
// 16 B of key per record while the batch is keyed; during the call four u64 arrays, the sort's temporary storage and the new
// record array.  Scratch comes from the library's grow-only scratch, the new records from the pool.
#include <memory>

#include "mg_collate_core.h"
#include "mg_internal.h"

namespace mg {

// hi[i] = the key's second half, idx[i] = i
__global__ __launch_bounds__(256) void k_collate_split(const uint64_t* __restrict__ keys2, uint64_t n, uint64_t* __restrict__ hi,
                                                       uint64_t* __restrict__ idx) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    hi[i] = keys2[2 * i + 1];
    idx[i] = i;
  }
}

// lo[j] = the first half of the key of record perm[j]
__global__ __launch_bounds__(256) void k_collate_lo(const uint64_t* __restrict__ keys2, const uint64_t* __restrict__ perm, uint64_t n,
                                                    uint64_t* __restrict__ lo) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) lo[j] = keys2[2 * perm[j]];
}

// Kernel A, first half: head[j] = j where the record at sorted position j opens a run of equal 128-bit keys, 0 elsewhere
// (position 0 opens one, and 0 is the identity of the max-scan that follows).
__global__ __launch_bounds__(256) void k_collate_heads(const uint64_t* __restrict__ keys2, const uint64_t* __restrict__ perm, uint64_t n,
                                                       uint64_t* __restrict__ head) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    bool opens = j == 0;
    if (!opens) {
      const uint64_t a = perm[j], b = perm[j - 1];
      opens = keys2[2 * a] != keys2[2 * b] || keys2[2 * a + 1] != keys2[2 * b + 1];  // BOTH halves decide
    }
    head[j] = opens ? j : 0;
  }
}

// Kernel A, second half: the run's head position -> the group id (the head's record index: the read's first retained line)
// and the final key.
__global__ __launch_bounds__(256) void k_collate_fkey(const uint64_t* __restrict__ perm, const uint64_t* __restrict__ headpos,
                                                      const mg_aln_rec* __restrict__ recs, uint64_t n, uint64_t* __restrict__ fkey) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    const uint64_t gid = perm[headpos[j]];
    fkey[j] = mgc::final_key(gid, recs[perm[j]].flag_len & MG_REC_FLAG_MASK);
  }
}

// Kernel B: out[t] = recs[perm[t]], its new-read bit recomputed from the sorted final keys.
__global__ __launch_bounds__(256) void k_collate_gather(const mg_aln_rec* __restrict__ recs, const uint64_t* __restrict__ perm,
                                                        const uint64_t* __restrict__ fkey, uint64_t n, mg_aln_rec* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
    const uint4 v = *reinterpret_cast<const uint4*>(recs + perm[t]);
    const bool opens = t == 0 || (fkey[t] >> 2) != (fkey[t - 1] >> 2);
    uint4 o = v;
    o.x = (v.x & MG_REC_REF_MASK) | (opens ? MG_REC_NEW_BIT : 0u);
    *reinterpret_cast<uint4*>(out + t) = o;
  }
}

// ... and a placed batch's places the same way: out[t] = place[perm[t]]
__global__ __launch_bounds__(256) void k_collate_gather_places(const mg_aln_place* __restrict__ place, const uint64_t* __restrict__ perm,
                                                               uint64_t n, mg_aln_place* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) out[t] = place[perm[t]];
}

// ... and its edits (MG_BATCH_EDITS)
__global__ __launch_bounds__(256) void k_collate_gather_edits(const mg_aln_edit* __restrict__ edit, const uint64_t* __restrict__ perm,
                                                              uint64_t n, mg_aln_edit* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) out[t] = edit[perm[t]];
}

// ... and its entries (MG_BATCH_BASES): 16 bytes each; the pool they point into stays where it is
__global__ __launch_bounds__(256) void k_collate_gather_bases(const mg_aln_bases* __restrict__ ent, const uint64_t* __restrict__ perm,
                                                              uint64_t n, mg_aln_bases* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) out[t] = ent[perm[t]];
}

// keys and flags -> d_perm[t] = the index of the record that comes t-th; *d_fkey (optional) = the sorted final keys (scratch:
// valid until the next collation).  n > 0.
static int collate_order(const uint64_t* d_keys2, const mg_aln_rec* d_recs, uint64_t n, uint64_t* d_perm, const uint64_t** d_fkey) {
  Context& c = ctx();
  hipStream_t st = c.stream;
  if (n >> 61) return fail(MG_ERR_ARG, "too many records to collate");
  uint64_t* A = (uint64_t*)scratch("col_a", n * sizeof(uint64_t));
  uint64_t* B = (uint64_t*)scratch("col_b", n * sizeof(uint64_t));
  uint64_t* C = (uint64_t*)scratch("col_c", n * sizeof(uint64_t));
  uint64_t* D = (uint64_t*)scratch("col_d", n * sizeof(uint64_t));
  if (!A || !B || !C || !D) return MG_ERR_NOMEM;
  const dim3 grid(grid_for(n, 256, (unsigned)c.num_cus * 16)), block(256);
  ProfScope ps("collate");
  // (hi, index) -> D = the indices by hi; (lo of those, D) -> B = the indices by (lo, hi, index)
  hipLaunchKernelGGL(k_collate_split, grid, block, 0, st, d_keys2, n, A, B);
  MG_HIP(hipGetLastError());
  MG_TRY(sort_pairs_u64(A, C, B, D, n, 64));
  hipLaunchKernelGGL(k_collate_lo, grid, block, 0, st, d_keys2, D, n, A);
  MG_HIP(hipGetLastError());
  MG_TRY(sort_pairs_u64(A, C, D, B, n, 64));
  // run heads -> group ids -> the final key
  hipLaunchKernelGGL(k_collate_heads, grid, block, 0, st, d_keys2, B, n, A);
  MG_HIP(hipGetLastError());
  MG_TRY(inclusive_max_u64(A, C, n));
  hipLaunchKernelGGL(k_collate_fkey, grid, block, 0, st, B, C, d_recs, n, A);
  MG_HIP(hipGetLastError());
  unsigned bits = 2;  // gid < n
  while (bits < 64 && ((n - 1) >> (bits - 2))) ++bits;
  MG_TRY(sort_pairs_u64(A, C, B, d_perm, n, bits));
  if (d_fkey) *d_fkey = C;
  return MG_OK;
}

int collate_batch(mg_sam_batch* b, uint64_t* d_perm_or_null) {
  if (!b->keyed) return fail(MG_ERR_STATE, "the batch carries no keys (tokenise it with a keyed call; a batch is collated once)");
  if (b->named) return fail(MG_ERR_STATE, "a named batch is not collated (its names are in the order the reads came in)");
  hipStream_t st = ctx().stream;
  const uint64_t n = b->nrecs;
  if (n) {
    uint64_t* d_perm = d_perm_or_null ? d_perm_or_null : (uint64_t*)scratch("col_perm", n * sizeof(uint64_t));
    if (!d_perm) return MG_ERR_NOMEM;
    const uint64_t* d_fkey = nullptr;
    MG_TRY(collate_order(b->keys.as<uint64_t>(), b->recs.as<mg_aln_rec>(), n, d_perm, &d_fkey));
    DevBuf out;  // (until here a failure leaves the batch as it was)
    MG_TRY(out.alloc((n + 1) * sizeof(mg_aln_rec)));
    DevBuf out_places;
    if (b->placed) {
      MG_TRY(out_places.alloc((n + 1) * sizeof(mg_aln_place)));
      hipLaunchKernelGGL(k_collate_gather_places, dim3(grid_for(n, 256, (unsigned)ctx().num_cus * 16)), dim3(256), 0, st,
                         b->places.as<mg_aln_place>(), d_perm, n, out_places.as<mg_aln_place>());
      MG_HIP(hipGetLastError());
    }
    DevBuf out_edits;
    if (b->edited) {
      MG_TRY(out_edits.alloc((n + 1) * sizeof(mg_aln_edit)));
      hipLaunchKernelGGL(k_collate_gather_edits, dim3(grid_for(n, 256, (unsigned)ctx().num_cus * 16)), dim3(256), 0, st,
                         b->edits.as<mg_aln_edit>(), d_perm, n, out_edits.as<mg_aln_edit>());
      MG_HIP(hipGetLastError());
    }
    DevBuf out_bases;
    if (b->based) {
      MG_TRY(out_bases.alloc((n + 1) * sizeof(mg_aln_bases)));
      hipLaunchKernelGGL(k_collate_gather_bases, dim3(grid_for(n, 256, (unsigned)ctx().num_cus * 16)), dim3(256), 0, st,
                         b->bases.as<mg_aln_bases>(), d_perm, n, out_bases.as<mg_aln_bases>());
      MG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_collate_gather, dim3(grid_for(n, 256, (unsigned)ctx().num_cus * 16)), dim3(256), 0, st, b->recs.as<mg_aln_rec>(),
                       d_perm, d_fkey, n, out.as<mg_aln_rec>());
    MG_HIP(hipGetLastError());
    MG_HIP(hipStreamSynchronize(st));
    b->recs = std::move(out);
    if (b->placed) b->places = std::move(out_places);
    if (b->edited) b->edits = std::move(out_edits);
    if (b->based) b->bases = std::move(out_bases);
  }
  b->keys.release();
  b->keyed = false;
  return MG_OK;
}

}  // namespace mg

using namespace mg;

extern "C" {

int mg_sam_tokenize_keyed_dev(const uint8_t* d_text, uint64_t nbytes, int paf, const mg_acc_index* ix, const char* prev_qname,
                              mg_sam_batch** out, int* err_kind, uint64_t* err_line) {
  return aln_tokenize_prefix_dev(d_text, nbytes, ix, prev_qname, paf != 0, true, nullptr, out, err_kind, err_line, false, true);
}

int mg_sam_batch_keys_download(const mg_sam_batch* b, uint64_t* keys2) {
  MG_REQUIRE_READY();
  if (!b || (b->nrecs && !keys2)) return fail(MG_ERR_ARG, "null argument");
  if (!b->keyed) return fail(MG_ERR_STATE, "the batch carries no keys");
  if (b->nrecs) MG_TRY(mg_memcpy_d2h(keys2, b->keys.p, b->nrecs * 2 * sizeof(uint64_t)));
  return MG_OK;
}

int mg_collate_order_dev(const uint64_t* d_keys2, const mg_aln_rec* d_recs, uint64_t n, uint64_t* d_perm) {
  MG_REQUIRE_READY();
  if (n == 0) return MG_OK;
  if (!d_keys2 || !d_recs || !d_perm) return fail(MG_ERR_ARG, "null argument");
  MG_TRY(collate_order(d_keys2, d_recs, n, d_perm, nullptr));
  MG_HIP(hipStreamSynchronize(ctx().stream));
  return MG_OK;
}

int mg_sam_batch_collate_dev(mg_sam_batch* b, uint64_t* d_perm_or_null) {
  MG_REQUIRE_READY();
  if (!b) return fail(MG_ERR_ARG, "null batch");
  return collate_batch(b, d_perm_or_null);
}

}  // extern "C"
