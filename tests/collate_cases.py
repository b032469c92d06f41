"""Shared by the collation tests (CPU and -m gpu): the two generated files of the issue's opening table put into coordinate
order, and the QNAMEs the key function is checked on."""
import random

import samgen

SEED = 0x6D67636F  # mg_collate_core.h: kSeed

KEY_NAMES = ([b"q" * n for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 254)]
             + [b"read/1234567890abcdefghijklmnopqrstuvwxyz"[:n] for n in (1, 5, 8, 9, 16, 17, 24, 33, 41)]  # prefixes of one another
             + [b"r" * 15 + c for c in (b"a", b"b")] + [b"s" * 32 + c for c in (b"a", b"b")]             # the last byte only
             + [b"t" * 253 + c for c in (b"0", b"1")] + [b"pair7", b"pair70", b"pair700"])


def case(nsingle, npairs):
    """-> (dbinfo text, accessions, acc_index, name-grouped SAM text)"""
    dbinfo, accs, taxids = samgen.make_dbinfo()
    acc_index = {"Unmapped": 0}
    acc_index.update({a: i + 1 for i, a in enumerate(accs)})
    text = samgen.make_sam_single(3, nsingle, accs, taxids, readlen=60) + samgen.make_sam_paired(4, npairs, accs, taxids)
    return dbinfo, accs, acc_index, text


def coordinate_shuffle(text, so="coordinate"):
    """The file as `samtools sort` leaves it: POS drawn from Random(11), the alignment lines sorted by (RNAME, POS) — stable, so
    equal coordinates keep their order — and the @HD line saying so."""
    rng = random.Random(11)
    head, body = [], []
    for ln in text.splitlines(True):
        if ln.startswith("@"):
            head.append(ln.replace("SO:unsorted", "SO:" + so) if ln.startswith("@HD") else ln)
            continue
        f = ln.split("\t")
        f[3] = str(rng.randrange(1, 40000))
        body.append(f)
    body.sort(key=lambda f: (f[2], int(f[3])))
    return head + ["\t".join(f) for f in body]
