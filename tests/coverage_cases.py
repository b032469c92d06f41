"""Shared by the coverage tests (CPU and -m gpu): seeded SAM text whose lines lie all over their references.

samgen's lines all start at POS 1000.  dress() gives a text `@SQ` lines for most accessions (not all), with lengths that differ
from db_info's, and rewrites POS — and now and then the CIGAR — of every alignment line: inside the reference, over its end,
beyond it, POS 0, CIGARs that consume no reference base, X / N / D ops."""
import random

import samgen
from metalign_amd import map_and_profile as mp


def tables(dbinfo_text):
    """db_info text -> (acc2info, taxid2info), as map_and_profile.get_acc2info reads the file."""
    acc2info, taxid2info = {}, {}
    for row in dbinfo_text.splitlines()[1:]:
        acc, acclen, taxid, namelin, taxlin = row.split("\t")
        rank = mp.get_taxid_rank(taxlin)
        if rank == "strain" and acc != "Unmapped":
            taxid, taxlin = taxid + ".1", taxlin + ".1"
        acc2info[acc] = [int(acclen), taxid, namelin, taxlin]
        taxid2info.setdefault(taxid, [0, rank, namelin, taxlin])[0] += int(acclen)
    return acc2info, taxid2info


def sq_lengths(accs, acc2info):
    """The `@SQ` lengths: every accession but each fifth, db_info's length moved by a few hundred either way."""
    return {a: acc2info[a][0] + (137 * (i + 1)) % 901 - 450 for i, a in enumerate(accs) if i % 5 != 4}


def dress(text, accs, acc2info, seed):
    """-> the lines of `text` with the `@SQ` header and varied POS / CIGAR (its own @SQ lines dropped, every other line kept)."""
    rng = random.Random(seed)
    sq = sq_lengths(accs, acc2info)
    head = [ln for ln in text.splitlines(True) if ln.startswith("@") and not ln.startswith("@SQ")]
    head += ["@SQ\tSN:%s\tLN:%d\n" % (a, n) for a, n in sq.items()]
    body = []
    for ln in text.splitlines(True):
        if ln.startswith("@"):
            continue
        f = ln.rstrip("\n").split("\t")
        if f[2] != "*" and f[5] != "*":
            L = sq.get(f[2], acc2info[f[2]][0])
            n = 40 if f[9] == "*" else len(f[9])
            u = rng.random()
            if u < 0.05:
                f[3] = "0"
            elif u < 0.10:
                f[3] = str(L + rng.randrange(1, 50))       # pos0 >= L
            elif u < 0.13:
                f[3] = str(L)                              # the last base: pos0 = L - 1
            elif u < 0.20:
                f[3] = str(L - rng.randrange(0, n))        # runs over the end
            else:
                f[3] = str(rng.randrange(1, L - n))
            v = rng.random()
            if v < 0.04:
                f[5] = "10S30I"                            # counts at pct_id 0 only; consumes no reference base
            elif v < 0.10:
                f[5] = "%dM%dX%dM" % (n - 12, 2, 10)
            elif v < 0.16:
                f[5] = "%dM%dN%dM" % (n // 2, rng.randrange(50, 400), n - n // 2)
            elif v < 0.22:
                f[5] = "%dM%dD%dM" % (n // 2, rng.randrange(1, 9), n - n // 2)
        body.append("\t".join(f) + "\n")
    return head + body


def case(nsingle, npairs, seed=21):
    """-> (db_info text, accessions, acc2info, taxid2info, acc_index, dressed lines)"""
    dbinfo, accs, taxids = samgen.make_dbinfo()
    acc2info, taxid2info = tables(dbinfo)
    acc_index = {"Unmapped": 0}
    acc_index.update({a: i + 1 for i, a in enumerate(accs)})
    text = samgen.make_sam_single(5, nsingle, accs, taxids, readlen=60) + samgen.make_sam_paired(6, npairs, accs, taxids)
    return dbinfo, accs, acc2info, taxid2info, acc_index, dress(text, accs, acc2info, seed)
