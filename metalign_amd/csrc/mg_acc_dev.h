// mg_acc_dev.h — the look-up of a name in the accession table on the device, shared by the parsers of text in HBM (mg_ingest.hip:
// SAM and PAF; mg_refseq.hip: the reference FASTA by record): ONE copy, device-only.
//
//   AccTable      the device's view of an mg_acc_index (acc_table_of)
//   acc_lookup()  a name's accession row, or -1: what the SAM tokeniser resolves RNAME with and the reference parser a record's name
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mg_internal.h"

namespace mg {

__device__ __forceinline__ uint64_t fnv1a(const uint8_t* p, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}

struct AccTable {
  const uint64_t* slot_hash;   // 0 = empty
  const uint32_t* slot_row;
  uint64_t mask;               // slots - 1
  const uint8_t* names;        // concatenated accession strings
  const uint64_t* name_off;    // [nacc + 1]
};

inline AccTable acc_table_of(const mg_acc_index* ix) {
  return AccTable{ix->slot_hash.as<uint64_t>(), ix->slot_row.as<uint32_t>(), ix->slots - 1, ix->names.as<uint8_t>(),
                  ix->name_off.as<uint64_t>()};
}

__device__ __forceinline__ int64_t acc_lookup(const AccTable& t, const uint8_t* s, uint32_t n) {
  uint64_t h = fnv1a(s, n);
  if (h == 0) h = 1;
  for (uint64_t p = h & t.mask;; p = (p + 1) & t.mask) {
    const uint64_t sh = t.slot_hash[p];
    if (sh == 0) return -1;
    if (sh == h) {
      const uint32_t row = t.slot_row[p];
      const uint64_t b = t.name_off[row], e = t.name_off[row + 1];
      if (e - b == n) {
        bool same = true;
        for (uint32_t i = 0; i < n && same; ++i) same = t.names[b + i] == s[i];
        if (same) return row;
      }
    }
  }
}

}  // namespace mg
