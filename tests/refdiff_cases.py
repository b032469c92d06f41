"""Shared by the reference tests (CPU and -m gpu): FASTA texts by record for refseq.py / mg_refseq.hip, and counts beside reference
codes for refdiff.py / mg_variants_diff, with the hand-worked expectations written out.
"""
import random

from metalign_amd import variants as var

LETTERS = b"ACGTN"  # the letter a reference code is written as (4: any byte that is no A, C, G or T)

# ---- records: the hand table ----------------------------------------------------------------------------------------------------
# rows a 0 (4 bases), b 1 (3), c 2 (0), d 3 (2), e 4 (5).
HAND_INDEX = {"a": 0, "b": 1, "c": 2, "d": 3, "e": 4}
HAND_LENGTHS = [4, 3, 0, 2, 5]
HAND_TEXT = (b"ACGT\n"            # in front of the first header: dropped
             b">a first\n"         # a: the name ends at the space
             b"AC\r\n"             # CRLF: the \r is stripped
             b"\n"                 # an empty line
             b"  g t \t\n"         # stripped at both ends only: the blank INSIDE stays and is coded 4 -> a has 5 bases: mismatched
             b">zz\n"              # foreign
             b"ACGT\n"
             b">b\tx\n"            # the name ends at the tab
             b"aNg\n"              # lower case, IUPAC: 0 4 2 -> b is loaded
             b">c\r\n"             # the name ends at the \r; no bases: c (length 0) is loaded
             b">d\x0bq\n"          # ... at the \v
             b"R\n"
             b" >x\n"              # its first byte is a blank: a sequence line, ">x" is two bases -> d has 3: mismatched
             b">d\x0c\n"           # ... at the \f; d again: duplicate, although this one has the right length
             b"AC\n"
             b">\n"                # an empty name: foreign
             b"AAAA\n"
             b"> e\n"              # the name is empty too (a blank right behind the `>`): foreign
             b">a\n"               # a again: duplicate (its first record mismatched)
             b"ACGT\n"
             b">e trailing header, no bases, no newline")  # e needs 5: mismatched
HAND_CODES = {1: bytes([0, 4, 2]), 2: b""}
HAND_LOADED = [0, 1, 1, 0, 0]
HAND_COUNTERS = (10, 2, 3, 3, 2)  # records, loaded (b, c), foreign (zz, "", ""), mismatched (a, d, e), duplicate (d, a)
HAND_RECORDS = [(b"a", b"ACg t"), (b"zz", b"ACGT"), (b"b", b"aNg"), (b"c", b""), (b"d", b"R>x"), (b"d", b"AC"), (b"", b"AAAA"),
                (b"", b""), (b"a", b"ACGT"), (b"e", b"")]

EDGE_TEXTS = {
    "empty": b"",
    "newline_only": b"\n",
    "no_header": b"ACGT\nACGT\n",
    "headers_only": b">r0\n>r1\n>zz\n>r2\n",
    "header_last_line": b">r1\nACGTAC\n>r0",
    "header_last_line_newline": b">r1\nACGTAC\n>r0\n",
    "no_final_newline": b">r1\nACG\nTAC",
    "crlf": b">r1 x\r\nACG\r\nTAC\r\n>r2\r\nAC\r\n",
    "one_line_each": b">r2\nAC\n>r1\nACGTAC\n>r0\n\n",
}
EDGE_NAMES, EDGE_LENGTHS = ["r0", "r1", "r2"], [0, 6, 2]

RECORD_LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 70001]
LINE_WIDTHS = [1, 15, 16, 17, 59, 60, 61, 80]


def bases(rng, n):
    """n bytes: mostly ACGT, some lower case, some IUPAC and other bytes (never white space, `>` or a newline)."""
    pool = b"ACGT" * 6 + b"acgt" + b"NRYn*-."
    return bytes(rng.choice(pool) for _ in range(n))


def wrap(seq, width):
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def geometry(width, lengths=RECORD_LENGTHS, seed=0):
    """-> (text, names, lengths): row i is record `lengths[i]` bases long; the FASTA holds the rows in REVERSED order, lines of
    `width` bases, and between the loaded records a foreign one, a mismatched one (row `short`, one base too many) and a duplicate
    of a loaded row, so that a wrong rank or record number shifts everything behind it."""
    rng = random.Random(seed * 1000 + width)
    names = ["row%d" % i for i in range(len(lengths))] + ["short"]
    lens = list(lengths) + [7]
    seqs = [bases(rng, n) for n in lens]
    text = [b"leading line, dropped\n"]
    for k, i in enumerate(reversed(range(len(lengths)))):
        text.append(b">" + names[i].encode() + b" rec %d\n" % k + wrap(seqs[i], width))
        if k == 1:
            text.append(b">other.%d\n" % width + wrap(bases(rng, 3 * width + 1), width))
        if k == 3:
            text.append(b">short\n" + wrap(seqs[-1] + b"A", width))
        if k == 5:
            text.append(b">" + names[i].encode() + b"\n" + wrap(seqs[i], width))
        if k == 6:
            text.append(b">short\n" + wrap(seqs[-1], width))  # the right length, but its row is taken: duplicate
    return b"".join(text), names, lens


# ---- the comparison: site classes under (D, C, F) = (5, 2, 50) -------------------------------------------------------------------
# (n4, r) -> (compared, ref_other, con_sub, pop_sub, emitted, ALT codes)
CLASSES = [
    (([1, 0, 0, 0], 0), (0, 0, 0, 0, 0, [])),         # not callable
    (([5, 0, 0, 0], 4), (0, 1, 0, 0, 0, [])),         # the reference is no A, C, G or T
    (([6, 0, 0, 0], 0), (1, 0, 0, 0, 0, [])),         # the sample is the reference
    (([0, 6, 0, 0], 0), (1, 0, 1, 1, 1, [1])),        # another base throughout
    (([2, 5, 0, 0], 0), (1, 0, 1, 0, 1, [1])),        # the major allele differs, the reference is a variant allele
    (([5, 2, 0, 0], 0), (1, 0, 0, 0, 1, [1])),        # polymorphic, the reference is the major allele
    (([3, 3, 3, 0], 3), (1, 0, 1, 1, 1, [0, 1, 2])),  # three alleles tie: A is major, ALT in code order
    (([0, 2, 3, 3], 0), (1, 0, 1, 1, 1, [2, 3, 1])),  # G before T on a tie, C last
    (([0, 0, 9, 1], 2), (1, 0, 0, 0, 0, [])),         # T has one read: below min_count
]
P = var.Params(5, 2, 50)
LOW = var.Params(2, 1, 0)
EDGE_POSITIONS = [62, 63, 64, 65, 1022, 1023, 1024, 1025]


def class_counts(lengths, shifts, quiet=()):
    """-> ({row: {pos: n4}}, {row: codes}): site pos of row j is class (pos + shifts[j]) % len(CLASSES); rows of one length whose
    shifts run through 0 .. len(CLASSES) - 1 put every class at every position.  The `quiet` rows get no count."""
    counts, ref = {}, {}
    for row, L in enumerate(lengths):
        ref[row] = bytes(CLASSES[(pos + shifts[row]) % len(CLASSES)][0][1] for pos in range(L))
        if row not in quiet:
            counts[row] = {pos: list(CLASSES[(pos + shifts[row]) % len(CLASSES)][0][0]) for pos in range(L)}
    return counts, ref


def fasta_of(names, ref, skip=(), width=60):
    """{row: codes} -> FASTA bytes (the rows in `skip` left out)."""
    return b"".join(b">" + names[r].encode() + b"\n" + wrap(bytes(LETTERS[c] for c in codes), width)
                    for r, codes in ref.items() if r not in skip)
