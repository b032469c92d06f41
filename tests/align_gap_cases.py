"""Seeded generators for the tests of the aligner's gapped extension (--align_band; metalign_amd/align.py: extend_gapped is the
definition): the reads of tests/align_cases.py with reads that need an insertion or a deletion added, at every read length, gap
length and gap position where the band, the tile of remembered bits or an accession's end can go wrong; and the planted-indel
property's reads.  table(band) builds the case table once and keeps the definition's answer beside it."""
import functools
import random
from collections import namedtuple

import align_cases as ac
from metalign_amd import align

K, W = 15, 5
BANDS = [1, 8, 31]
LENGTHS = [K, 63, 64, 65, 150, 151, 1024]


def gap_params_of(band):
    return align.gap_params(band=band)


def with_deletion(genome, at, L, where, g):
    """L read bases from genome[at:], the g reference bases behind read base `where` left out."""
    return genome[at:at + where] + genome[at + where + g:at + L + g]


def with_insertion(rng, genome, at, L, where, g):
    """L read bases: g random bases in front of read base `where`, the other L - g from genome[at:]."""
    return genome[at:at + where] + ac.rand_seq(rng, g) + genome[at + where:at + L - g]


def gap_reads(t, band, seed):
    """-> [(name, sequence)]: the reads with gaps, beside the table's own."""
    rng = random.Random(seed)
    g = {name: seq for name, seq in t.rows}
    big, other, noisy, tandem, rep = g["len70001"], g["len5000"], g["noisy"], g["tandem"], g["repeat"]
    out, n = [], [0]

    def add(name, seq):
        n[0] += 1
        out.append((name, ac.revcomp(seq) if n[0] % 2 else seq))  # (every other read on the other strand)

    # every gap length and position at 150 bases; the other lengths with one gap of each kind in the middle and one base from an end
    for L in LENGTHS:
        sizes = sorted({1, band, band + 1}) if L == 150 else [band]
        for size in sizes:
            if size + 4 > L:
                continue
            spots = sorted({0, 1, 2, L // 2, L - size - 2, L - size - 1, L - size} if L == 150 else {L // 2, L - size - 1})
            for where in spots:
                if where < 0 or where + size > L:
                    continue
                at = rng.randrange(100, len(big) - 2 * L - 100)
                add("del_L%d_g%d_at%d" % (L, size, where), with_deletion(big, at, L, where, size))
                at = rng.randrange(100, len(big) - 2 * L - 100)
                add("ins_L%d_g%d_at%d" % (L, size, where), with_insertion(rng, big, at, L, where, size))
    # hanging over either end of the accession by 1, by k and by more than the band, with a gap in the middle: cells with j < 0, j >= n
    L = 150
    for over in (1, K, band + 5):
        left = ac.rand_seq(rng, over) + with_deletion(big, 0, L - over, 70, min(band, 3))
        right = with_insertion(rng, big, len(big) - (L - over) + 2, L - over, 70, 2) + ac.rand_seq(rng, over)
        add("gap_left%d" % over, left)
        add("gap_leftrc%d" % over, left)
        add("gap_right%d" % over, right)
        add("gap_rightrc%d" % over, right)
    # the gap itself at the accession's first and last bases
    add("del_at_start", big[0:2] + big[3:151])
    add("del_at_end", big[-150:-3] + big[-2:])
    # longer than its accession
    for name in ("len63", "len64", "len65"):
        short = g[name]
        add("longer_" + name, ac.rand_seq(rng, 30) + short[:30] + short[31:] + ac.rand_seq(rng, 30))
        add("longer_ins_" + name, ac.rand_seq(rng, 5) + short[:30] + b"G" + short[30:] + ac.rand_seq(rng, 5))
    # across two rows adjacent in memory (len5000, then len70001), a gap in each half: the band must not see the neighbour
    add("across_gaps", other[-77:-40] + other[-38:] + big[:40] + big[43:78])
    add("across_gaps2", other[-60:-4] + other[-3:] + big[1:90])
    add("across_ins", other[-75:-1] + b"A" + other[-1:] + big[:75])
    # N and lower case beside the gap, in the read and in the reference
    seq = bytearray(with_deletion(big, 20000, 150, 75, 2))
    seq[74:76] = b"NN"
    seq[60:74] = bytes(seq[60:74]).lower()
    add("read_n_at_gap", bytes(seq))
    seq = bytearray(with_insertion(rng, big, 21000, 150, 75, 3))
    seq[75:78] = b"NnN"
    add("read_n_inserted", bytes(seq))
    add("ref_lower_del", noisy[520:598] + noisy[601:673])  # the reference is lower case from 600 on
    add("ref_n_del", noisy[930:999] + noisy[1003:1080])    # the deleted bases hold the reference's N at 1000 and 1001
    add("ref_n_ins", noisy[930:1000] + b"AC" + noisy[1000:1078])
    add("ref_n_run", noisy[230:299] + noisy[352:433])      # the N run 300 .. 349 longer than any band
    add("ref_iupac", noisy[1150:1199] + noisy[1201:1300])
    # the tandem and repeat rows: ties, and refined alignments that collapse
    add("tandem_del", tandem[700:770] + tandem[773:853])
    add("tandem_ins", tandem[700:770] + b"ACG" + tandem[770:847])
    add("tandem_unit", tandem[640:760] + tandem[800:830])  # one whole unit of 40 left out
    add("tie_del", rep[520:590] + rep[592:672])
    add("tie_ins", rep[510:590] + b"T" + rep[590:659])
    # homopolymers: the tie rule places the gap
    homo = big[30000:30070] + big[30075:30150]
    add("plain_del5", homo)
    # two gaps in one read
    add("two_gaps", big[40000:40050] + big[40003 + 50:40100] + b"GT" + big[40100:40151])
    add("two_dels", big[41000:41040] + big[41041:41090] + big[41092:41160])
    add("two_ins", big[42000:42040] + b"C" + big[42040:42090] + b"AA" + big[42090:42147])
    assert len({x for x, _ in out}) == len(out)
    return out


GapTable = namedtuple("GapTable", "t gp reads alns stats_of")


@functools.lru_cache(maxsize=None)
def table(band):
    """The case table of (K, W) with its own reads and the gapped ones, and the definition's answers at this band:
    alns[name] = the kept alignments, stats_of[name] = (distinct, accepted, refined candidates)."""
    t = ac.table(K, W)
    gp = gap_params_of(band)
    reads = list(t.reads) + gap_reads(t, band, 4000 + band)
    assert len({name for name, _ in reads}) == len(reads)
    alns, stats_of = {}, {}
    for name, seq in reads:
        kept, ncand, nacc, nref = align.align_read_gapped(seq, t.index, t.ref, t.p, gp)
        alns[name], stats_of[name] = kept, (ncand, nacc, nref)
    return GapTable(t, gp, reads, alns, stats_of)


def batch_of(gt, n):
    """n reads of the table, in turn -> (names, sequences, kept alignments per read, align.Stats, refined candidates)."""
    picks = [gt.reads[i % len(gt.reads)] for i in range(n)]
    names, seqs = [x[0] for x in picks], [x[1] for x in picks]
    alns = [gt.alns[x] for x in names]
    stats = align.Stats(n, sum(1 for x in alns if x), sum(gt.stats_of[x][0] for x in names), sum(gt.stats_of[x][1] for x in names),
                        sum(len(x) for x in alns))
    return names, seqs, alns, stats, sum(gt.stats_of[x][2] for x in names)


def unrefined_reads(t, n=70):
    """Reads no candidate of which is refined: exact copies of the big genome, whose ungapped segment is the whole read."""
    big = dict(t.rows)["len70001"]
    return [big[1000 + 137 * i:1150 + 137 * i] for i in range(n)]


# ---- the planted-indel property (tests/test_align_gap_host.py; the GPU test aligns the same reads) ----------------------------------
PROPERTY_BAND, PROPERTY_SUB, PROPERTY_SEED = 8, 0.02, 11


@functools.lru_cache(maxsize=None)
def property_inputs(sub=PROPERTY_SUB, seed=PROPERTY_SEED, band=PROPERTY_BAND):
    """3 random genomes of 20 000 bases and 300 reads of 150 bases.  Read r is drawn uniformly from a genome with ONE indel of
    1 .. band bases (uniform) planted `where` bases into it, 20 <= where <= 130 (uniform): even r a deletion (that many reference
    bases left out), odd r an insertion (that many random bases put in); then every base is substituted with probability `sub`;
    reads with r % 4 >= 2 are reverse-complemented.  -> (names, lengths, fasta, ref, reads [(name, seq)], truth [accession row])."""
    rng = random.Random(seed)
    genomes = [ac.rand_seq(rng, 20000) for _ in range(3)]
    names = ["g%d" % i for i in range(3)]
    fasta = ac.fasta_of(list(zip(names, genomes)), width=60)
    ref = ac.refseq.parse(fasta, {n: i for i, n in enumerate(names)}, [20000] * 3)
    reads, truth = [], []
    for r in range(300):
        a = rng.randrange(3)
        size, where = rng.randrange(1, band + 1), rng.randrange(20, 131)
        at = rng.randrange(0, 20000 - 150 - band + 1)
        if r % 2 == 0:
            seq = bytearray(with_deletion(genomes[a], at, 150, where, size))
        else:
            seq = bytearray(with_insertion(rng, genomes[a], at, 150, min(where, 150 - size), size))
        assert len(seq) == 150
        for j in range(150):
            if rng.random() < sub:
                seq[j] = rng.choice([c for c in b"ACGT" if c != seq[j]])
        reads.append(("read%d" % r, ac.revcomp(bytes(seq)) if r % 4 >= 2 else bytes(seq)))
        truth.append(a)
    return names, [20000] * 3, fasta, ref, reads, truth


def found(kept, a):
    """A read counts as found when its primary lies on the right accession and covers at least 140 read bases."""
    return bool(kept) and kept[0].a == a and kept[0].e - kept[0].b >= 140
