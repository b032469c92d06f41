"""Shared by the identity tests (CPU and -m gpu): a hand table that covers every rule of metalign_amd/identity.py, and seeded SAM
text whose tags vary — NM in front of, behind and between other tags of every type, twice, missing, of another type, out of range.

dress() rewrites the tags of samgen's alignment lines.  With bam_safe=True every tag can be written to a BAM record by bamgen and
means the same there as in the text; bam_safe=False adds values only text can hold (an empty NM:i:, leading zeros, a sign, twelve
digits, a malformed value)."""
import random

import samgen
from coverage_cases import tables

# (the tables of test_coverage_host.py / test_depth_host.py)
A2I = {"Unmapped": [0, "Unmapped", "", ""], "c1": [1000, "g1.1", "", ""], "c2": [1000, "g1.1", "", ""], "c3": [1000, "g1.1", "", ""],
       "d1": [500, "g2", "", ""]}
T2I = {"Unmapped": [0], "g1.1": [3000], "g2": [500]}


def L(q, flag, rname, cigar, tags, seq="ACGT"):
    return "\t".join([q, str(flag), rname, "1", "60", cigar, "*", "0", "0", seq, "*"] + list(tags)) + "\n"


# The twelfth field must be a tag whose value int() takes (the tokeniser raises otherwise), so a malformed NM stands behind one.
HAND = [
    "@HD\tVN:1.6\n",
    "@SQ\tSN:c1\tLN:1000\n",
    L("a", 0, "c1", "10M", ["NM:i:0"]),                              # NM the twelfth field
    L("b", 0, "c1", "10M", ["AS:i:20", "ms:i:3", "NM:i:1"]),         # behind other tags
    L("c", 0, "c1", "10M", ["NM:i:2", "NM:i:9"]),                    # two: the first wins
    L("d", 0, "c1", "10M", ["AS:i:1", "NM:i:"]),                     # empty: unscored
    L("e", 0, "c1", "10M", ["NM:i:-1"]),                             # negative: unscored
    L("f", 0, "c1", "10M", ["NM:i:+3"]),                             # a sign
    L("g", 0, "c1", "100M", ["NM:i:0007"]),                          # leading zeros
    L("h", 0, "c1", "10M", ["NM:i:123456789012"]),                   # twelve digits: too large, unscored
    L("i", 0, "c1", "10M", ["NM:Z:3"]),                              # another type: unscored
    L("j", 0, "c1", "10M", ["nm:i:3"]),                              # lower case: unscored
    L("k", 0, "c2", "10M", ["NM:i:25"]),                             # NM above cols: e = cols
    L("l", 0, "c2", "10S5N", ["NM:i:0"]),                            # cols 0: counts at pct_id 0 only, unscored there
    L("m", 0, "c2", "5M2I3D4X6M", ["NM:i:9"]),                       # I, D and X: cols 20, matched 11 of 20
    L("n", 2048, "c1", "10M", ["NM:i:0"]),                           # supplementary: does not count
    L("o", 0, "c1", "4M6S", ["NM:i:0"]),                             # 0.4: below pct_id 0.5
    L("p", 256, "d1", "10M", ["NM:i:1"], seq="*"),                   # a secondary counts
    L("q", 4, "c1", "10M", ["NM:i:0"]),                              # unmapped: not retained
    L("r", 0, "c1", "10M", ["AS:i:1", "NM:i:4294967294"]),           # the largest usable value
    L("s", 0, "c1", "10M", ["AS:i:1", "NM:i:4294967295"]),           # one more: unscored
    L("t", 0, "d1", "10M", ["NM:i:-0"]),                             # int('-0') = 0
    L("u", 0, "c1", "10M", ["AS:i:5", "XNM:i:3", "NM:i:1x", "NM:i:0"]),  # malformed, and the search stops there: unscored
    L("v", 0, "c1", "10M5m", ["NM:i:1"]),                            # a lower-case op is of no kind: cols 10
    b"w\t0\td1\t1\t60\t8M\t*\t0\t0\tACGT\t*\tNM:i:0\n",              # bytes
    "x\t0\td1\t1\t60\t10M\t*\t0\t0\tACGT\t*\tAS:i:3  \x1fNM:i:4 \n",  # split on str.split()'s white space
]

_MIDDLE = ["ms:i:-5", "AS:i:77", "XA:A:x", "tp:A:P", "XF:f:1.5", "XZ:Z:hello", "XZ:Z:a b NM:i:77 c", "XH:H:1AE3", "XB:B:c,1,-2",
           "XB:B:C,200", "XB:B:s,-300,4", "XB:B:S,1,2,3", "XB:B:i,-70000", "XB:B:I,5", "XB:B:f,1.5,2.5", "XB:B:C", "XS:i:300",
           "XL:i:-70000", "XI:i:3000000000", "XW:Z:x\x1fy", "NX:i:4", "XN:Z:NM:i:5"]
_NM_SAFE = ["NM:Z:3", "NM:A:3", "NM:f:3", "NM:i:-1", "NM:i:70000", "NM:i:4294967295", "NM:i:4294967294", "NM:i:300", "NM:H:1A",
            "NM:B:c,3"]
_NM_TEXT = ["NM:i:", "NM:i:0007", "NM:i:+2", "NM:i:123456789012", "NM:i:1x", "NM:i:-", "NM:i:99999999999999999999999", "NM:i:-0"]


def tags_for(rng, bam_safe=True):
    """One line's tags; the first one always has a value int() takes."""
    u = rng.random()
    nm = "NM:i:%d" % rng.choice([0, 0, 0, 1, 1, 2, 3, 5, 9, 40])
    if u < 0.45:
        tags = [nm] + rng.sample(_MIDDLE, rng.randrange(0, 4))
    elif u < 0.75:
        tags = [rng.choice(["AS:i:60", "XZ:Z:7", "ms:i:-3", "tp:A:1"])] + rng.sample(_MIDDLE, rng.randrange(0, 5)) + [nm]
        if rng.random() < 0.3:
            tags += ["NM:i:17"] + rng.sample(_MIDDLE, 1)
    elif u < 0.85:  # none at all
        tags = ["AS:i:60"] + rng.sample(_MIDDLE, rng.randrange(0, 6))
    else:
        odd = rng.choice(_NM_SAFE if bam_safe else _NM_SAFE + 2 * _NM_TEXT)
        tags = ["AS:i:60"] + rng.sample(_MIDDLE, rng.randrange(0, 3)) + [odd] + ([nm] if rng.random() < 0.5 else [])
    return tags


def dress(text, seed, bam_safe=True):
    """-> the lines of `text` with every alignment line's tags (and now and then its CIGAR) drawn anew."""
    rng = random.Random(seed)
    out = []
    for ln in text.splitlines(True):
        if ln.startswith("@"):
            out.append(ln)
            continue
        f = ln.rstrip("\n").split("\t")
        n = 40 if f[9] == "*" else len(f[9])
        if f[5] != "*":
            v = rng.random()
            if v < 0.04:
                f[5] = "%dS%dN" % (n // 2, n)             # no column; counts at pct_id 0 only
            elif v < 0.12:
                f[5] = "%dM2X%dM" % (n - 12, 10)
            elif v < 0.2:
                f[5] = "%dM3I%dM4D" % (n // 2, n - n // 2 - 3)
        out.append("\t".join(f[:11] + tags_for(rng, bam_safe)) + "\n")
    return out


def case(nsingle, npairs, seed=41, bam_safe=True):
    """-> (db_info text, accessions, acc2info, taxid2info, acc_index, dressed lines): a few accessions of two taxids take most of
    the lines (samgen's skew), the rest are spread."""
    dbinfo, accs, taxids = samgen.make_dbinfo()
    acc2info, taxid2info = tables(dbinfo)
    acc_index = {"Unmapped": 0}
    acc_index.update({a: i + 1 for i, a in enumerate(accs)})
    text = samgen.make_sam_single(7, nsingle, accs, taxids, readlen=60) + samgen.make_sam_paired(8, npairs, accs, taxids)
    return dbinfo, accs, acc2info, taxid2info, acc_index, dress(text, seed, bam_safe)
