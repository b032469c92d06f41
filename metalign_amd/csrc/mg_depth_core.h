// mg_depth_core.h — the arithmetic of per-base depth (--depth, --depth_windows; metalign_amd/depth.py is the definition): what the
// depth kernels (mg_depth.hip) decide per slot.
//
//   slots          accession a of length L owns L + 1 int32 slots at a 64-bit offset: slot p < L takes +1 for every interval that
//                  starts at p and -1 for every one that ends there, slot L the -1 of the intervals that end at L.  So an
//                  accession's slots sum to zero, and ONE inclusive scan over all slots leaves depth[p] in slot p (and 0 in every
//                  accession's extra slot) without segment flags.
//   slots_of()     L + 1
//   diff_slots()   the two slots an interval [pos0, pos0 + clen) of accession a touches
//   is_base()      slot s of the accession at `off` with length L is a base (not the extra slot)
//   clamp()        min(depth, kDepthCap): the histogram's bin
//   window_of()    the window of position p at width W; windows_of_length(): ceil(L / W)
//   tiles_of()     the scan's tiles over n slots; tile_has_row(): must the passes read this tile at all
// The accession of a slot or window is mgv::owner_of / mgv::owner_from (mg_coverage_core.h).
//
// Written so that the SAME code compiles for the host (tests/host_depth_check.cpp) and for gfx950.
#pragma once
#include <stdint.h>

#include "mg_coverage_core.h"

namespace mgd {

constexpr uint32_t kDepthCap = 4095, kDepthBins = kDepthCap + 1;
constexpr uint32_t kTile = 1024;  // slots per scan tile: 256 threads, one int4 each

using mgv::owner_of;  // the accession of a slot or window (moved to mg_coverage_core.h for the coverage and variants kernels)

MGV_HD uint64_t slots_of(uint64_t L) { return L + 1; }
MGV_HD void diff_slots(uint64_t off, uint32_t pos0, uint64_t clen, uint64_t* plus, uint64_t* minus) {
  *plus = off + pos0;
  *minus = off + pos0 + clen;
}
MGV_HD bool is_base(uint64_t s, uint64_t off, uint64_t L) { return s - off < L; }
MGV_HD uint32_t clamp(uint32_t depth) { return depth < kDepthCap ? depth : kDepthCap; }
MGV_HD uint64_t window_of(uint64_t p, uint32_t W) { return p / W; }
MGV_HD uint64_t windows_of_length(uint64_t L, uint32_t W) { return W ? (L + W - 1) / W : 0; }
MGV_HD uint64_t tiles_of(uint64_t nslots) { return (nslots + kTile - 1) / kTile; }

// Does an accession with a histogram row (rowmap >= 0) own a slot of the tile that ends at s_end?  a = the accession of the tile's
// first slot.  Without one, every slot of the tile is zero and so is every depth in it: neither pass has to read it.
template <class O, class R> MGV_HD bool tile_has_row(const O& off, const R& rowmap, uint32_t nacc, uint32_t a, uint64_t s_end) {
  for (uint32_t b = a; b < nacc && off[b] < s_end; ++b)
    if (rowmap[b] >= 0) return true;
  return false;
}

}  // namespace mgd
