"""Seeded generators for the tests of the aligner's paired-end mode (--align_pairs interleaved; metalign_amd/align.py: rescue_pair and
select_pair are the definition): a small reference, interleaved pairs at every mate length, fragment length, orientation and
accession edge where the rescue window, the concordance test or the pair choice can go wrong, and the rescue property's pairs.
answers(I, R, band) aligns the case table once per parameter set and keeps the definition's answer beside it; the host tests and
the GPU tests share it."""
import functools
import random
from collections import namedtuple

import align_cases as ac
from metalign_amd import align, refseq

K, W = 15, 5
LENGTHS = [K, 63, 64, 65, 150, 1024]
# (max_insert, rescue, band): the defaults with and without the band; no rescue; one anchor; windows of exactly 1, 63, 64 and 65
# diagonals for two mates of 150 bases (I - 149); the largest insert, with every anchor
PARAM_SETS = [(1000, 2, 0), (1000, 2, 8), (1000, 0, 8), (1000, 1, 0), (150, 2, 0), (212, 2, 0), (213, 2, 8), (214, 2, 0), (8192, 2, 0),
              (8192, 8, 8)]


def unseedable(seq, phase=5):
    """seq with a substitution at every 12th base: no run of 15 bases survives, so no 15-mer seeds."""
    out = bytearray(seq)
    for j in range(phase, len(out), 12):
        out[j] = ord({65: "C", 67: "G", 71: "T", 84: "A"}[out[j]])
    return bytes(out)


def mates(genome, at, F, L1, L2, flip=False):
    """The two mates of the fragment genome[at:at + F]: mate 1 its first L1 bases, mate 2 the reverse complement of its last L2;
    flip: the other way round (mate 1 is the one on strand 1)."""
    frag = genome[at:at + F]
    first, second = (L2, L1) if flip else (L1, L2)
    fwd, rev = frag[:first], ac.revcomp(frag[F - second:])
    return (rev, fwd) if flip else (fwd, rev)


@functools.lru_cache(maxsize=None)
def reference(seed=31):
    """-> [(name, sequence)]: `big` for the long inserts, `mid` and `next` adjacent in memory, `tandem` with 12 copies of a unit of
    40, and `twinA` / `twinB`, which share their first 400 bases."""
    rng = random.Random(seed)
    shared = ac.rand_seq(rng, 400)
    unit = ac.rand_seq(rng, 40)
    return [("big", ac.rand_seq(rng, 12000)), ("mid", ac.rand_seq(rng, 5000)), ("next", ac.rand_seq(rng, 3000)),
            ("tandem", ac.rand_seq(rng, 600) + unit * 12 + ac.rand_seq(rng, 600)),
            ("twinA", shared + ac.rand_seq(rng, 1600)), ("twinB", shared + ac.rand_seq(rng, 1600)), ("tiny", ac.rand_seq(rng, 200))]


def pairs_for(rows, seed=32):
    """-> [(name, mate 1, mate 2)]: the names are distinct."""
    rng = random.Random(seed)
    g = dict(rows)
    big, mid, nxt, tandem, twin_a, tiny = g["big"], g["mid"], g["next"], g["tandem"], g["twinA"], g["tiny"]
    out = []

    def add(name, pair, unseed=None):
        m1, m2 = pair
        if unseed == 1:
            m1 = unseedable(m1)
        if unseed == 2:
            m2 = unseedable(m2)
        out.append((name, m1, m2))

    # proper pairs, both orientations; the fragment exactly the insert limits of the parameter sets, and one base longer
    for F in (150, 151, 212, 213, 214, 215, 400, 1000, 1001, 8192, 8193):
        for flip in (False, True):
            at = rng.randrange(100, len(big) - F - 100)
            add("proper_F%d_%d" % (F, flip), mates(big, at, F, 150, 150, flip))
            at = rng.randrange(100, len(big) - F - 100)
            add("rescue2_F%d_%d" % (F, flip), mates(big, at, F, 150, 150, flip), unseed=2)
            at = rng.randrange(100, len(big) - F - 100)
            add("rescue1_F%d_%d" % (F, flip), mates(big, at, F, 150, 150, flip), unseed=1)
    # every pair of mate lengths (L != L' in both directions; a mate inside the other: the fragment as long as the longer mate)
    for L1 in LENGTHS:
        for L2 in LENGTHS:
            F = max(L1, L2) + (0 if (L1 + L2) % 2 else 137)
            at = rng.randrange(100, len(big) - F - 100)
            add("len_%d_%d" % (L1, L2), mates(big, at, F, L1, L2, flip=(L1 + L2) % 4 == 0), unseed=2 if L2 >= 63 else None)
            if L1 >= 63:
                at = rng.randrange(100, len(big) - F - 100)
                add("len1_%d_%d" % (L1, L2), mates(big, at, F, L1, L2), unseed=1)
    # a mate at the accession's first and last base: the window is clipped; and hanging over it: negative diagonals
    add("first_base", mates(mid, 0, 400, 150, 150), unseed=1)
    add("last_base", mates(mid, len(mid) - 400, 400, 150, 150), unseed=2)
    add("first_base_flip", mates(mid, 0, 300, 150, 150, flip=True), unseed=2)
    add("last_base_flip", mates(mid, len(mid) - 300, 300, 150, 150, flip=True), unseed=1)
    m1, m2 = mates(mid, 0, 380, 150, 150)
    out.append(("hang_left", unseedable(ac.rand_seq(rng, 12) + m1[:138]), m2))
    m1, m2 = mates(mid, len(mid) - 380, 380, 150, 150)
    out.append(("hang_right", m1, unseedable(ac.rand_seq(rng, 12) + m2[:138])))
    # the window would cross into the next accession (mid, then next, adjacent in memory): mate 2 lies on `next`, 300 bases on
    add("cross_next", (mid[len(mid) - 200:len(mid) - 50], ac.revcomp(nxt[150:300])), unseed=2)
    add("cross_prev", (ac.revcomp(nxt[50:200]), mid[len(mid) - 300:len(mid) - 150]), unseed=2)
    add("tiny_window", mates(tiny, 10, 180, 150, 150), unseed=2)
    # the tandem repeat: the unseedable mate scores equally on diagonals 40 apart, the smallest wins
    add("tandem_rescue", (tandem[300:450], ac.revcomp(tandem[700:850])), unseed=2)
    add("tandem_rescue_flip", (ac.revcomp(tandem[1150:1300]), tandem[700:850]), unseed=2)
    add("tandem_both", (tandem[640:790], ac.revcomp(tandem[840:990])))
    # mate 1 inside the repeat is accepted on diagonals 40 apart: two anchors whose windows both hold mate 2's place
    add("two_anchors", (tandem[700:850], ac.revcomp(tandem[1150:1300])), unseed=2)
    # mate 1 on both twins equally, mate 2 on twinA alone: the pair settles the multimapped mate
    add("twin_settled", (twin_a[100:250], ac.revcomp(twin_a[500:650])))
    add("twin_both", (twin_a[50:200], ac.revcomp(twin_a[220:370])))  # both mates on both twins: two proper pairs
    add("twin_rescue", (twin_a[100:250], ac.revcomp(twin_a[500:650])), unseed=2)
    # a rescued mate that needs the band: a deletion of 3 and an insertion of 2 in the unseedable mate
    m1, m2 = mates(big, 3000, 500, 150, 153)
    out.append(("rescue_del", m1, unseedable(m2[:80] + m2[83:])))
    m1, m2 = mates(big, 3600, 500, 150, 148)
    out.append(("rescue_ins", m1, unseedable(m2[:70] + b"AC" + m2[70:])))
    m1, m2 = mates(big, 4200, 450, 153, 150, flip=True)
    out.append(("rescue_del_flip", unseedable(m1[:60] + m1[63:]), m2))
    # a seeded candidate just outside the window: mate 2 seeds 5 bases beyond the insert limit of 1000 (no task at band 8, one at 0)
    add("seeded_near", mates(big, 5000, 1005, 150, 150))
    add("seeded_far", mates(big, 6000, 1040, 150, 150))
    # the mates on different accessions, on one strand, and the wrong way round: no proper pair
    add("two_accessions", (big[700:850], ac.revcomp(mid[900:1050])))
    add("same_strand", (big[800:950], big[1100:1250]))
    add("outward", (ac.revcomp(big[900:1050]), big[1200:1350]))
    # unaligned mates
    add("mate1_unaligned", (ac.rand_seq(rng, 150), ac.revcomp(big[2000:2150])))
    add("mate2_unaligned", (big[2100:2250], ac.rand_seq(rng, 150)))
    add("both_unaligned", (ac.rand_seq(rng, 150), ac.rand_seq(rng, 150)))
    add("mate2_short", (big[2300:2450], ac.revcomp(big[2500:2500 + K - 1])))
    add("mate2_long", (big[2600:2750], ac.revcomp(big[2800:2800 + 1025])))
    add("mate1_empty", (b"", ac.revcomp(big[2900:3050])))
    # lower case and N in the rescued mate
    m1, m2 = mates(big, 7000, 420, 150, 150)
    out.append(("rescue_lower_n", m1, unseedable(m2).lower()[:75] + b"N" + unseedable(m2)[76:]))
    assert len({n for n, _, _ in out}) == len(out)
    return out


Table = namedtuple("Table", "p names lengths rows fasta ref index pairs")


@functools.lru_cache(maxsize=None)
def table():
    rows = reference()
    names, lengths = [n for n, _ in rows], [len(s) for _, s in rows]
    fasta = ac.fasta_of(rows)
    ref = refseq.parse(fasta, {n: i for i, n in enumerate(names)}, lengths)
    p = align.params(k=K, w=W)
    return Table(p, names, lengths, rows, fasta, ref, align.build_index(ref, K, W), pairs_for(rows))


Answer = namedtuple("Answer", "gp pp kept proper counts")


@functools.lru_cache(maxsize=None)
def answers(max_insert, rescue, band):
    """The definition on every pair of the table under these parameters: kept[name] = (mate 1's kept alignments, mate 2's),
    proper[name], counts[name] = (distinct, accepted, refined, rescued candidates, tasks)."""
    t = table()
    gp, pp = align.gap_params(band), align.pair_params(1, max_insert, rescue)
    kept, proper, counts = {}, {}, {}
    for name, m1, m2 in t.pairs:
        k1, k2, pr, ncand, nacc, nref, nres, ntask = align.align_pair(m1, m2, t.index, t.ref, t.p, gp, pp)
        kept[name], proper[name], counts[name] = (k1, k2), pr, (ncand, nacc, nref, nres, ntask)
    return Answer(gp, pp, kept, proper, counts)


def batch_of(ans, names):
    """The pairs `names` of the table, in that order -> (sequences interleaved, kept alignments per read, proper per pair,
    align.Stats, align.PairStats)."""
    by_name = {n: (m1, m2) for n, m1, m2 in table().pairs}
    seqs, alns, proper = [], [], []
    for n in names:
        seqs += list(by_name[n])
        alns += list(ans.kept[n])
        proper.append(ans.proper[n])
    stats = align.Stats(len(seqs), sum(1 for x in alns if x), sum(ans.counts[n][0] for n in names), sum(ans.counts[n][1] for n in names),
                        sum(len(x) for x in alns))
    return seqs, alns, proper, stats, align.PairStats(sum(ans.counts[n][2] for n in names), sum(ans.counts[n][3] for n in names),
                                                      sum(proper))


def all_names():
    return [n for n, _, _ in table().pairs]


# ---- the rescue property (tests/test_align_pair_host.py; the GPU test aligns the same pairs) ---------------------------------------
@functools.lru_cache(maxsize=None)
def property_inputs(seed=5):
    """One random genome of 20 000 bases and 300 pairs of two mates of 150 bases from fragments of 300 .. 600 bases (uniform), the
    fragment's place uniform; mate 2 has a substitution at every 12th base, so none of its 15-mers survives; every other pair has
    mate 1 on strand 1.  -> (names, lengths, fasta, ref, sequences interleaved, truth [(d of mate 1, d of mate 2, flipped)])."""
    rng = random.Random(seed)
    genome = ac.rand_seq(rng, 20000)
    fasta = ac.fasta_of([("g0", genome)], width=60)
    ref = refseq.parse(fasta, {"g0": 0}, [20000])
    seqs, truth = [], []
    for r in range(300):
        F = rng.randrange(300, 601)
        at = rng.randrange(0, 20000 - F + 1)
        flip = r % 2 == 1
        m1, m2 = mates(genome, at, F, 150, 150, flip)
        seqs += [m1, unseedable(m2)]
        truth.append((at + F - 150, at, True) if flip else (at, at + F - 150, False))
    return ["g0"], [20000], fasta, ref, seqs, truth


def planted(k1, k2, proper, truth):
    """A pair counts when it is proper and both primaries lie on their planted diagonals and strands."""
    d1, d2, flip = truth
    return bool(proper and k1 and k2 and (k1[0].strand, k1[0].d) == (int(flip), d1) and (k2[0].strand, k2[0].d) == (1 - int(flip), d2))
