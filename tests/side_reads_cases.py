"""Shared by the --side_reads tests (CPU and -m gpu): synthetic records with synthetic verdict words, why the definition masks
each of them, and a small sample in which a close relative collects only the shared reads of a strain that is present."""
import numpy as np

import coverage_cases as cc
import samgen
from metalign_amd import _hip

TILE = 4096         # mgs::kTile (metalign_amd/csrc/mg_sidemask_core.h): the records per tile of the NEW-bit scan
SCAN_THREADS = 256  # kScanBlock (mg_sidemask.hip): the threads of the workgroup that scans the tile counts


def synthetic(n, seed, nreads_short=0, nref=6, ntax=2, p_new=0.4, first_new=True):
    """n synthetic records, synthetic verdict words of kinds 0 to 3 and a ref2tax: the mask is a pure function of them.  Three in a
    hundred records lie on row nref (at or above it); nreads_short: that many reads fewer than the records open."""
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, dtype=_hip.REC_DTYPE)
    new = rng.random(n) < p_new
    if n and first_new:
        new[0] = True
    rows = rng.integers(0, nref, n).astype(np.uint32)
    rows[rng.random(n) < 0.03] = nref
    recs["ref_new"] = rows | (new.astype(np.uint32) << np.uint32(31))
    recs["matched"] = rng.integers(1, 100, n)
    recs["total"] = 100
    recs["flag_len"] = rng.choice([0, 16, 256, 99, 147, 2048, 2064], n).astype(np.uint32) | np.uint32(60 << 12)
    nreads = max(int(new.sum()) - nreads_short, 0)
    kind = rng.choice([0, 0, 1, 1, 1, 1, 2, 3], nreads).astype(np.uint64)
    words = np.zeros(2 * nreads, dtype=np.uint64)
    words[0::2] = kind | (rng.integers(0, ntax, nreads).astype(np.uint64) << np.uint64(2)) * (kind == 1)
    words[1::2] = rng.integers(0, 1000, nreads)
    ref2tax = (np.arange(nref) % ntax).astype(np.uint32)
    return recs, words, ref2tax


def reasons(recs, words, ref2tax):
    """The share of the records that is kept, and that the rule masks for each reason, the reasons taken in the rule's order: the
    ordinal or the row out of bounds, the dropped first line, a read that is not unique, an accession of another taxon."""
    n, nreads, nref = len(recs), len(words) // 2, len(ref2tax)
    new = (recs["ref_new"] & np.uint32(_hip.NEW_BIT)) != 0
    row = (recs["ref_new"] & np.uint32(_hip.REF_MASK)).astype(np.int64)
    ordinal = np.cumsum(new) - 1
    out = dict(kept=0, bounds=0, dropped=0, kind=0, taxon=0)
    for i in range(n):
        o = int(ordinal[i])
        if o < 0 or o >= nreads or row[i] >= nref:
            out["bounds"] += 1
        elif new[i] and (o == 0 or int(words[2 * (o - 1)]) & 3 == 0):
            out["dropped"] += 1
        elif int(words[2 * o]) & 3 != 1:
            out["kind"] += 1
        elif int(ref2tax[row[i]]) != int(words[2 * o]) >> 2:
            out["taxon"] += 1
        else:
            out["kept"] += 1
    return {k: v / max(n, 1) for k, v in out.items()}


# ---- a sample: two strains with two accessions each that are present, and a relative that is not -----------------------------------
ACCS = ["NZ_A1.1", "NZ_A2.1", "NZ_B1.1", "NZ_B2.1", "NZ_REL.1"]
RELATIVE = "NZ_REL.1"
_TAXA = {"NZ_A1.1": (0, 0), "NZ_A2.1": (0, 0), "NZ_B1.1": (1, 0), "NZ_B2.1": (1, 0), "NZ_REL.1": (0, 1)}  # (species, strain)


def sample(nsingle=1500, nrelative=80, npairs=800):
    """-> (db_info text, lines).  samgen's single-end and paired reads over the four accessions of the two strains that are present
    (unique, multimapped, ambiguous, filtered, supplementary); between them reads of strain A whose secondary alignment lies on
    the relative, a second strain of A's species: multimapped every one, so no read is ever uniquely the relative's."""
    rows, taxids = [], []
    for acc in ACCS:
        sp, st = _TAXA[acc]
        names = ["Bacteria", "Phy1", "Cls1", "Ord1", "Fam1", "Genus1", "Genus1 species%d" % sp, "Genus1 species%d str. %d" % (sp, st)]
        ids = ["2", "101", "201", "301", "401", "501", str(1000 + sp), str(900000 + 10 * sp + st)]
        rows.append("\t".join([acc, "50000", ids[-1], "|".join(names), "|".join(ids)]) + "\n")
        taxids.append(ids[-1])
    dbinfo = samgen.DBINFO_HEADER + samgen.UNMAPPED_ROW + "".join(rows)
    present, present_tax = ACCS[:4], taxids[:4]
    text = samgen.make_sam_single(31, nsingle, present, present_tax, readlen=60)
    seq = "ACGT" * 15
    # (two lines, so multimapped or — its first line dropped — unique, never ambiguous: the first relative read keeps its primary)
    text += samgen._line("pre", 0, "NZ_B1.1", "60M", seq, 0) + samgen._line("pre", 256, "NZ_B2.1", "60M", "*", 1)
    for i in range(nrelative):
        text += samgen._line("rel%d" % i, 0, ACCS[i % 2], "60M", seq, 0) + samgen._line("rel%d" % i, 256, RELATIVE, "60M", "*", 2)
    text += samgen.make_sam_paired(32, npairs, present, present_tax)
    acc2info, _ = cc.tables(dbinfo)
    return dbinfo, cc.dress(text, ACCS, acc2info, 33)
