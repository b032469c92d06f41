"""Shared by the variants tests (CPU and -m gpu): a hand table that covers every rule of metalign_amd/variants.py with every count
written out by hand, the site rule at its edges, and seeded SAM text whose reads pile up on a few hundred sites.

HAND_WANT[i] is what HAND[i] says by itself (variants.bases_of): (pos0, span, codes), or None for a line that is not retained.
"""
import random
import struct

import identity_cases as ic

# lengths: c1 20, c2 1000, d1 8 (no @SQ line overrides them)
A2I = {"Unmapped": [0, "Unmapped", "", ""], "c1": [20, "g1.1", "", ""], "c2": [1000, "g1.1", "", ""], "d1": [8, "g2", "", ""]}
T2I = {"Unmapped": [0], "g1.1": [1020], "g2": [8]}
ACC_INDEX = {"Unmapped": 0, "c1": 1, "c2": 2, "d1": 3}
NOT_PILED = (0, 0, [])


def L(q, flag, rname, pos, cigar, seq, tags=("NM:i:0",)):
    return "\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "*"] + list(tags)) + "\n"


_TABLE = [
    ("@HD\tVN:1.6\n", None),
    (L("a", 0, "c1", 1, "5M", "ACGTA"), (0, 5, [0, 1, 2, 3, 0])),
    (L("b", 0, "c1", 1, "2S3M", "TTACG"), (0, 3, [0, 1, 2])),                  # S consumes query bases only
    (L("c", 0, "c1", 2, "2M1I2M", "ACTGT"), (1, 4, [0, 1, 2, 3])),              # I likewise: the T is stepped over
    (L("d", 0, "c1", 1, "2M2D2M", "ACGT"), (0, 6, [0, 1, 5, 5, 2, 3])),         # D: two GAP codes
    (L("e", 0, "c1", 1, "2M3N2M", "ACGT"), (0, 7, [0, 1, 5, 5, 5, 2, 3])),      # N: three
    (L("f", 0, "c1", 3, "3M2H", "CCC"), (2, 3, [1, 1, 1])),                     # H consumes nothing
    (L("g", 0, "c1", 1, "3M2m", "ACG"), (0, 3, [0, 1, 2])),                     # a lower-case op is of no kind (total is 5: 0.6)
    (L("h", 0, "c1", 1, "5M", "*"), NOT_PILED),                                 # SEQ *
    (L("i", 0, "c1", 1, "5M", "ACGT"), NOT_PILED),                              # one base too short
    (L("j", 0, "c1", 1, "5M", "ACGTAC"), NOT_PILED),                            # one base too long
    (L("k", 0, "c1", 0, "5M", "ACGTA"), NOT_PILED),                             # POS 0
    (L("l", 0, "c1", "1x", "5M", "ACGTA"), NOT_PILED),                          # POS not digits
    (L("m", 0, "c1", 18, "5M", "GGGGG"), (17, 5, [2, 2, 2, 2, 2])),             # across L = 20: clipped to 3 sites
    (L("n", 0, "c1", 21, "5M", "GGGGG"), (20, 5, [2, 2, 2, 2, 2])),             # pos0 == L: unpiled (the line itself can be piled)
    (L("p", 0, "c2", 1, "5M", "NRaCg"), (0, 5, [4, 4, 0, 1, 2])),               # N and R are OTHER, lower case counts
    (L("q", 2048, "c1", 1, "5M", "TTTTT"), (0, 5, [3, 3, 3, 3, 3])),            # FLAG 2048: does not count
    (L("r", 0, "c1", 1, "2M3S", "TTTTT"), (0, 2, [3, 3])),                      # 0.4: just below pct_id 0.5, does not count
    (L("s", 16, "c1", 1, "5M", "TTTTT"), (0, 5, [3, 3, 3, 3, 3])),              # FLAG 16 counts, SEQ as it stands
    (L("t", 4, "c1", 1, "5M", "TTTTT"), None),                                  # unmapped: not retained
    (b"u\t0\td1\t8\t60\t1M1X\t*\t0\t0\tAC\t*\tNM:i:1\n", (7, 2, [0, 1])),       # bytes; X emits a base; clipped to 1 site
]
HAND = [ln for ln, _ in _TABLE]
HAND_WANT = [w for _, w in _TABLE]

# What the hand table piles at pct_id 0.5, site by site (a b c d e f g m s count and pile on c1; h i j k l n are unpiled):
#   c1 site 0: A of a b d e g, T of s             site 1: C of a b d e g, A of c, T of s      site 2: G of a b g, C of c f, T of s
#      site 3: T of a s, G of c, C of f           site 4: A of a, T of c s, G of d, C of f    site 5: T of d, G of e     site 6: T of e
#      sites 17 18 19: G of m
HAND_COUNTS = {
    "c1": {0: [5, 0, 0, 1], 1: [1, 5, 0, 1], 2: [0, 2, 3, 1], 3: [0, 1, 1, 2], 4: [1, 1, 1, 2], 5: [0, 0, 1, 1], 6: [0, 0, 0, 1],
           17: [0, 0, 1, 0], 18: [0, 0, 1, 0], 19: [0, 0, 1, 0]},
    "c2": {2: [1, 0, 0, 0], 3: [0, 1, 0, 0], 4: [0, 0, 1, 0]},
    "d1": {7: [1, 0, 0, 0]},
}
HAND_ALIGNMENTS = {"c1": 9, "c2": 1, "d1": 1}
HAND_UNPILED = 6
# D = 5, C = 2, F = 50: sites 0, 1, 2 and 4 of c1 are callable (d = 6, 7, 6, 5; site 3 has d = 4)
#   site 0: pairs 30, same 5 * 4 = 20             -> discordant 10;  T has 1 < C
#   site 1: pairs 42, same 20                     -> 22
#   site 2: pairs 30, same 2 + 6 = 8              -> 22; major G, C has 2 >= C and 2000 >= 50 * 6: polymorphic
#   site 4: pairs 20, same 2                      -> 18; major T (2), nobody else has 2
HAND_PER = {"c1": [9, 4, 1, 122, 72], "c2": [1, 0, 0, 0, 0], "d1": [1, 0, 0, 0, 0]}
HAND_SITES = [("c1", 2, (0, 2, 3, 1))]
# pi = 72 / 122 = 0.590163..., snv_per_kb = 1000 * 1 / 4
HAND_FILE = ("#kind\tid\ttaxid\tlength\talignments\tcallable_sites\tpolymorphic_sites\tpairs\tdiscordant_pairs\tpi\tsnv_per_kb\n"
             "#min_depth\t5\tmin_count\t2\tmin_freq_permille\t50\n"
             "S\tc1\tg1.1\t20\t9\t4\t1\t122\t72\t0.590164\t250.000000\n"
             "S\tc2\tg1.1\t1000\t1\t0\t0\t0\t0\t0.000000\t0.000000\n"
             "S\td1\tg2\t8\t1\t0\t0\t0\t0\t0.000000\t0.000000\n"
             "G\tg1.1\tg1.1\t1020\t10\t4\t1\t122\t72\t0.590164\t250.000000\n"
             "G\tg2\tg2\t8\t1\t0\t0\t0\t0\t0.000000\t0.000000\n"
             "#unpiled\t6\n")
HAND_SITES_FILE = ("#accession\tpos\tdepth\tA\tC\tG\tT\tmajor\tvariant_alleles\n"
                   "#min_depth\t5\tmin_count\t2\tmin_freq_permille\t50\n"
                   "c1\t3\t6\t0\t2\t3\t1\tG\tC\n")

# A span of exactly MAX_PILE_SPAN and one above: such a line counts only at pct_id 0 (an M that long would need a SEQ above 2^20 - 1
# bases, which the tokeniser refuses)
SPAN_MAX = L("v", 0, "c2", 1, "1M2097150N", "A")
SPAN_OVER = L("w", 0, "c2", 1, "1M2097151N", "A")

# (n4, (D, C, F)) -> (callable, major, variant alleles, pairs, discordant)
SITE_CASES = [
    ([4, 0, 0, 0], (5, 2, 50), (False, 0, [], 0, 0)),            # d = D - 1
    ([5, 0, 0, 0], (5, 2, 50), (True, 0, [], 20, 0)),            # d = D
    ([5, 2, 0, 0], (5, 3, 0), (True, 0, [], 42, 20)),            # n_a = C - 1
    ([5, 3, 0, 0], (5, 3, 0), (True, 0, [1], 56, 30)),           # n_a = C
    ([18, 2, 0, 0], (5, 2, 100), (True, 0, [1], 380, 72)),       # 1000 n_a == F d
    ([19, 2, 0, 0], (5, 2, 100), (True, 0, [], 420, 76)),        # one below: 2000 < 2100
    ([3, 3, 0, 0], (5, 2, 50), (True, 0, [1], 30, 18)),          # a two-way tie: the lowest code is the major allele
    ([0, 3, 0, 3], (5, 2, 50), (True, 1, [3], 30, 18)),          # ... whichever codes tie
    ([2, 2, 2, 2], (5, 2, 50), (True, 0, [1, 2, 3], 56, 48)),    # a four-way tie
    ([100, 2, 0, 0], (5, 2, 0), (True, 0, [1], 10302, 400)),     # F = 0: the count alone decides
    ([100, 2, 0, 0], (5, 2, 50), (True, 0, [], 10302, 400)),     # ... 2000 < 5100
    ([0, 0, 0, 0], (2, 1, 0), (False, 0, [], 0, 0)),
    ([1, 1, 0, 0], (2, 1, 500), (True, 0, [1], 2, 2)),           # the smallest callable site, F at its largest
]


# ---- BAM records of the hand table (tests/host_variants_check.cpp, and the GPU test through bamgen) -----------------------------
_OPS = "MIDNSHP=X"
_NIB = "=ACMGRSVTWYHKDBN"


def bam_record(qname, flag, ref_id, pos0, cigar, seq):
    """One BAM record, block_size first, without aux fields: the record ends with its QUAL."""
    ops, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            ops.append((int(num) << 4) | _OPS.index(ch))
            num = ""
    seq = "" if seq == "*" else seq.upper()
    packed = bytearray((len(seq) + 1) // 2)
    for j, ch in enumerate(seq):
        packed[j >> 1] |= _NIB.index(ch) << (0 if j & 1 else 4)
    name = qname.encode() + b"\0"
    body = struct.pack("<iiBBHHHIiii", ref_id, pos0, len(name), 60, 0, len(ops), flag, len(seq), -1, -1, 0) + name
    body += b"".join(struct.pack("<I", o) for o in ops) + bytes(packed) + b"\xff" * len(seq)
    return struct.pack("<I", len(body)) + body


def hand_bam_cases():
    """[(record bytes, expected (pos0, span, codes), placed)] of the hand lines a BAM record can hold (no lower-case op, a POS of
    digits); placed = False: POS 0, which the tokeniser's place refuses before the core's walk is asked."""
    out = []
    for ln, want in _TABLE:
        if want is None or isinstance(ln, bytes):
            continue
        f = ln.rstrip("\n").split("\t")
        if not f[3].isdigit() or any(c.islower() for c in f[5]):
            continue
        out.append((bam_record(f[0], int(f[1]), 0, int(f[3]) - 1, f[5], f[9]), want, int(f[3]) >= 1))
    # an even l_seq with a soft clip in front, and all sixteen nibbles
    out.append((bam_record("x", 0, 0, 4, "2S14M", "=ACMGRSVTWYHKDBN"), (4, 14, [1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]), True))
    return out


# ---- seeded text ---------------------------------------------------------------------------------------------------------------
def dress(lines, seed, spread=120):
    """identity_cases' dressed lines with every alignment line's POS drawn anew — a pile-up of a few hundred sites around 1000, now
    and then at the end of a 50000-base accession (clipped) or behind it — and an N in a SEQ here and there."""
    rng = random.Random(seed)
    out = []
    for ln in lines:
        if ln.startswith("@"):
            out.append(ln)
            continue
        f = ln.rstrip("\n").split("\t")
        u = rng.random()
        f[3] = str(rng.randrange(49990, 50012) if u < 0.03 else 1000 + rng.randrange(spread))
        if f[9] != "*" and rng.random() < 0.2:
            at = rng.randrange(len(f[9]))
            f[9] = f[9][:at] + "N" + f[9][at + 1:]
        out.append("\t".join(f) + "\n")
    return out


def case(nsingle, npairs, seed=43):
    """-> identity_cases.case with dress() on top: (db_info text, accessions, acc2info, taxid2info, acc_index, lines)."""
    dbinfo, accs, acc2info, taxid2info, acc_index, lines = ic.case(nsingle, npairs, seed=seed, bam_safe=True)
    return dbinfo, accs, acc2info, taxid2info, acc_index, dress(lines, seed + 1)
