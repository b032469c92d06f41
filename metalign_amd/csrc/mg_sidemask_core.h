// mg_sidemask_core.h — which records the side outputs count under --side_reads unique (metalign_amd/side_reads.py is the
// definition: unique_lines over lines, unique_mask_of_records over records and verdict words): what the mask kernel
// (mg_sidemask.hip) decides per record.
//
//   kind_of()      the low two bits of a read's verdict word 0 (mg_profile_commit_assign_dev): 0 ambiguous, 1 unique, 2 multimapped,
//                  3 not counted; for kind 1 the dense taxon id lies above them
//   in_range()     the record's read ordinal — the records with MG_REC_NEW_BIT in [0, i], minus one — is one of the nreads reads the
//                  words speak of.  A stream whose first record is not NEW has ordinal -1 there: 2^64 - 1 as the u64 it is carried in
//   keep()         the record is evidence for the taxon stage C counted its read for.  Masked:
//                    * an ordinal outside [0, nreads), an accession row at or above nref (ref2tax is never read out of bounds);
//                    * the line the read loop drops (scripts/map_and_profile.py:229-232): a NEW record of read 0 (the phantom
//                      boundary) or of a read whose predecessor was ambiguous;
//                    * a record of a read that is not unique;
//                    * a record on an accession of another taxon than the read's.
//
// Written so that the SAME code compiles for the host (tests/host_sidemask_check.cpp) and for gfx950.  The verdict words are reached
// through an accessor (`w0[r]` = word 0 of read r).
#pragma once
#include <stdint.h>

#include "../../include/metalign_hip.h"
#include "mg_coverage_core.h"

namespace mgs {

constexpr uint32_t kTile = 4096;        // records per tile of the NEW-bit scan
constexpr uint32_t kMaskFlag = 2048u;   // the FLAG bit a masked record gets: mgv::counts() refuses it

MGV_HD uint32_t kind_of(uint64_t w0) { return (uint32_t)(w0 & 3ull); }
MGV_HD bool is_new(const mg_aln_rec& r) { return (r.ref_new & MG_REC_NEW_BIT) != 0; }
MGV_HD bool in_range(uint64_t ord, uint64_t nreads) { return ord < nreads; }

template <class W> MGV_HD bool keep(const mg_aln_rec& r, uint64_t ord, uint64_t nreads, const W& w0, const uint32_t* ref2tax,
                                    uint32_t nref) {
  const uint32_t row = r.ref_new & MG_REC_REF_MASK;
  if (!in_range(ord, nreads) || row >= nref) return false;
  if (is_new(r) && (ord == 0 || kind_of(w0[ord - 1]) == 0)) return false;
  const uint64_t mine = w0[ord];
  if (kind_of(mine) != 1) return false;
  return (uint64_t)ref2tax[row] == (mine >> 2);
}

MGV_HD mg_aln_rec masked(mg_aln_rec r) {
  r.flag_len |= kMaskFlag;
  return r;
}

}  // namespace mgs
