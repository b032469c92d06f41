"""Shared by the consensus tests (CPU and -m gpu): per-site counts written as span-1 records, the hand table of variants_cases with
the FASTA bytes it gives written out by hand, and the lengths and widths at which the text's layout can go wrong.
"""
import numpy as np

import variants_cases as vc
from metalign_amd import _hip
from metalign_amd import variants as var

IUPAC = "-ACMGRSVTWYHKDBN"

# ---- the hand table: variants_cases.HAND over A2I (c1 20, c2 1000, d1 8), whose counts are HAND_COUNTS ---------------------------
# (D, C, F) = (5, 2, 50): c1's sites 0, 1, 2 and 4 are callable (A, C, G, T); site 2 [0, 2, 3, 1] has the variant allele C: S
# (D, C, F) = (2, 1, 0): c1's sites 0 .. 5 are callable and all polymorphic:
#   0 [5, 0, 0, 1] A + T = W    1 [1, 5, 0, 1] C + A + T = H    2 [0, 2, 3, 1] G + C + T = B    3 [0, 1, 1, 2] T + C + G = B
#   4 [1, 1, 1, 2] all = N (major T)                5 [0, 0, 1, 1] a tie, G before T: G + T = K    6 and 17 .. 19 have d = 1: N
# c2 and d1 have no site of depth 2.
HAND_SEQ = {
    ((5, 2, 50), False): {"c1": "ACGNT" + "N" * 15, "c2": "N" * 1000, "d1": "N" * 8},
    ((5, 2, 50), True): {"c1": "ACSNT" + "N" * 15, "c2": "N" * 1000, "d1": "N" * 8},
    ((2, 1, 0), False): {"c1": "ACGTTGN" + "N" * 13, "c2": "N" * 1000, "d1": "N" * 8},
    ((2, 1, 0), True): {"c1": "WHBBNKN" + "N" * 13, "c2": "N" * 1000, "d1": "N" * 8},
}
HAND_CALLED = {(5, 2, 50): {"c1": (9, 4, 1), "c2": (1, 0, 0), "d1": (1, 0, 0)},   # alignments, called, ambiguous
               (2, 1, 0): {"c1": (9, 6, 6), "c2": (1, 0, 0), "d1": (1, 0, 0)}}
_TAIL = " min_depth=5 min_count=2 min_freq_permille=50 ambiguity=major"
_C2_TEXT = ("N" * 60 + "\n") * 16 + "N" * 40 + "\n"


def hand_file(extra=""):
    """The file of the hand table at the defaults, mode major; extra: what follows `ambiguity=major` in every header line."""
    return (">c1 taxid=g1.1 length=20 alignments=9 called=4 ambiguous=1" + _TAIL + extra + "\nACGNTNNNNNNNNNNNNNNN\n"
            ">c2 taxid=g1.1 length=1000 alignments=1 called=0 ambiguous=0" + _TAIL + extra + "\n" + _C2_TEXT +
            ">d1 taxid=g2 length=8 alignments=1 called=0 ambiguous=0" + _TAIL + extra + "\nNNNNNNNN\n").encode()


# ---- the layout: lengths and widths ---------------------------------------------------------------------------------------------
ROW_LENGTHS, ROW_WIDTH = list(range(1, 18)), 5   # in a row: every text starts at another residue mod 4 and mod 16
LENGTHS = [0, 59, 60, 61, 120, 121, 4096, 4097, 70001]
WIDTHS = [1, 3, 60, 61, 4096]
TEXT_WIDTHS = [1, 3, 60]


def text_lengths(w):
    return [0, 1, w - 1, w, w + 1, 2 * w, 2 * w + 1]


# ---- counts ---------------------------------------------------------------------------------------------------------------------
# With (D, C, F) = (2, 1, 0): the lowest allele of a mask twice, the others once — the major allele and its variants give the mask
MASK_CASES = {m: [(2 if (m & -m) == (1 << a) else 1) if (m >> a) & 1 else 0 for a in range(4)] for m in range(1, 16)}
# ... and d = D - 1, no read at all, two ties
PATTERNS = list(MASK_CASES.values()) + [[1, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [0, 1, 0, 1], [0, 0, 0, 1]]


def pattern_counts(lengths, quiet=()):
    """{row: {pos: n4}}: every site of every row (but the `quiet` rows) takes one of PATTERNS, so that neighbouring sites and
    neighbouring rows differ."""
    return {row: {pos: PATTERNS[(row * 7 + pos * 11 + pos // 20) % len(PATTERNS)] for pos in range(L)}
            for row, L in enumerate(lengths) if row not in quiet}


def records_of_counts(counts):
    """{row: {pos: n4}} -> recs, entries, pool: n4[k] records of span 1 and code k on every site (variants.pack: a byte each)."""
    recs, ent, pool = [], [], bytearray()
    for row, sites in counts.items():
        for pos, n4 in sites.items():
            for k in range(4):
                for _ in range(n4[k]):
                    recs.append((row, 10, 10, 40 << 12))
                    ent.append((len(pool), pos, 1))
                    pool += var.pack([k])
    return (np.array(recs, dtype=_hip.REC_DTYPE) if recs else np.zeros(0, dtype=_hip.REC_DTYPE),
            np.array(ent, dtype=_hip.BASES_DTYPE) if ent else np.zeros(0, dtype=_hip.BASES_DTYPE), bytes(pool))
