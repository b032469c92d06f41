// mg_align_gap_core.h — the per-cell rules of the aligner's gapped extension (--align_band; metalign_amd/align.py: extend_gapped is the
// definition): what k_al_gap of mg_align.hip decides per cell of the band, per candidate and per step of the walk back.
//
//   The cells of a candidate (oriented read o of L bases, accession codes g of n bases, diagonal d, band B) are (i, j) with
//   0 <= i < L, 0 <= j < n and t = j - i - d + B in [0, 2B]: row i, band offset t.  In a row the existing cells are contiguous in t.
//   Cell (i - 1, j - 1) is offset t of row i - 1, cell (i - 1, j) offset t + 1 of row i - 1, cell (i, j - 1) offset t - 1 of row i.
//
//   gap_sub()            s(i, j): +1 for a match of two codes below 4, else -P
//   gap_ins()            I(i, j) from H and I of cell (i - 1, j), kGapNone where that cell does not exist
//   gap_del()            D(i, j) from H and D of cell (i, j - 1): the rule as the definition states it, one cell after the other
//   gap_del_prefix()     D(i, j) from the largest H'(u) + u E over the offsets u < t of the row, H' = max(0, X, I): the same value
//                        (O >= 0: a gap opened from a D cell never beats the one opened from the H' cell that D came from)
//   gap_bits()           the four bits a cell remembers: where H came from (stop / diagonal / I / D), whether I opened, whether D opened
//   gap_best_pack()      (H, i, t) as one number whose maximum is the best cell: the largest H, then the smallest i, then the smallest j
//   GapWalk / gap_walk() the walk back, one remembered nibble at a time: diagonal before insertion before deletion, open before extend
//
// Written so that the SAME code compiles for the host (tests/host_align_gap_check.cpp) and for gfx950.
#pragma once
#include <stdint.h>

#include "mg_align_core.h"

namespace mga {

constexpr uint32_t kMaxBand = 31;            // a row of 2B + 1 <= 63 cells: one wavefront
constexpr int32_t kGapNone = -(1 << 29);     // no I / no D: below every value a cell can take, and far from overflow
constexpr uint32_t kSrcStop = 0, kSrcDiag = 1, kSrcIns = 2, kSrcDel = 3;  // H == X and the walk ends here / goes on; H == I; H == D
constexpr uint32_t kSrcMask = 3, kInsOpened = 4, kDelOpened = 8;
constexpr uint32_t kOpM = 0, kOpI = 1, kOpD = 2;  // a column of an alignment, one byte each in the kernel's workspace

MGA_HD int32_t gap_max(int32_t a, int32_t b) { return a > b ? a : b; }

MGA_HD int32_t gap_sub(uint32_t oc, uint32_t gc, int32_t P) { return oc < 4 && oc == gc ? 1 : -P; }

MGA_HD int32_t gap_ins(bool up_exists, int32_t h_up, int32_t i_up, int32_t O, int32_t E) {
  return up_exists ? gap_max(h_up - O - E, i_up - E) : kGapNone;
}

MGA_HD int32_t gap_del(bool left_exists, int32_t h_left, int32_t d_left, int32_t O, int32_t E) {
  return left_exists ? gap_max(h_left - O - E, d_left - E) : kGapNone;
}

// what offset u offers the offsets right of it; kGapNone for a cell that does not exist
MGA_HD int32_t gap_del_offer(bool exists, int32_t hq, int32_t u, int32_t E) { return exists ? hq + u * E : kGapNone; }

// pm: the largest offer of the offsets u < t (kGapNone: cell (i, j - 1) does not exist)
MGA_HD int32_t gap_del_prefix(int32_t pm, int32_t t, int32_t O, int32_t E) { return pm > kGapNone / 2 ? pm - O - t * E : kGapNone; }

MGA_HD int32_t gap_h(int32_t X, int32_t I, int32_t D) { return gap_max(gap_max(0, X), gap_max(I, D)); }

// h_diag: H(i - 1, j - 1), 0 where that cell does not exist; h_up / h_left: H of the cells I and D open from (anything where none)
MGA_HD uint32_t gap_bits(int32_t H, int32_t X, int32_t I, int32_t D, int32_t h_diag, int32_t h_up, int32_t h_left, int32_t O, int32_t E) {
  uint32_t bits = H == X ? (h_diag > 0 ? kSrcDiag : kSrcStop) : H == I ? kSrcIns : kSrcDel;
  if (I != kGapNone && I == h_up - O - E) bits |= kInsOpened;
  if (D != kGapNone && D == h_left - O - E) bits |= kDelOpened;
  return bits;
}

// H <= 1024, i < 1024, t < 64
MGA_HD uint32_t gap_best_pack(int32_t H, int32_t i, int32_t t) { return ((uint32_t)H << 16) | ((1023u - (uint32_t)i) << 6) | (63u - (uint32_t)t); }
MGA_HD int32_t gap_best_h(uint32_t key) { return (int32_t)(key >> 16); }
MGA_HD int32_t gap_best_i(uint32_t key) { return 1023 - (int32_t)((key >> 6) & 1023u); }
MGA_HD int32_t gap_best_t(uint32_t key) { return 63 - (int32_t)(key & 63u); }

struct GapWalk {
  int32_t i, t;        // the cell
  uint32_t state = 0;  // 0 H, 1 I, 2 D
  bool done = false;
};

// One step at cell (w.i, w.t) whose remembered bits are `nib` -> the column it emits (kOpM / kOpI / kOpD), or -1 for a change of
// state alone.  After an M column with w.done the walk has ended AT this cell: (w.i, w.t) is the alignment's first column.
MGA_HD int32_t gap_walk(GapWalk& w, uint32_t nib) {
  if (w.state == 0) {
    const uint32_t src = nib & kSrcMask;
    if (src == kSrcStop) {
      w.done = true;
      return (int32_t)kOpM;
    }
    if (src == kSrcDiag) {
      --w.i;
      return (int32_t)kOpM;
    }
    w.state = src == kSrcIns ? 1u : 2u;
    return -1;
  }
  if (w.state == 1) {
    w.state = (nib & kInsOpened) ? 0u : 1u;
    --w.i;
    ++w.t;
    return (int32_t)kOpI;
  }
  w.state = (nib & kDelOpened) ? 0u : 2u;
  --w.t;
  return (int32_t)kOpD;
}

}  // namespace mga
