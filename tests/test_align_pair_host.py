"""The aligner's paired-end mode on the host (--align_pairs interleaved; metalign_amd/align.py: rescue_pair, select_pair): cases whose
answer follows from how they were made, the old selection as a view of the pair lists, the records against the tokenised SAM text,
the flags and their refusals, mg_align_pair_core.h under the sanitizers against vectors the definition wrote, the rescue
property, and what a pair does to the profile."""
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import align_gap_cases as gc
import align_pair_cases as pc
from metalign_amd import align, assignments, cli, map_and_profile, metalign, refseq
from metalign_amd.side_outputs import align_pair_params, check_flags

HERE = os.path.dirname(os.path.abspath(__file__))
BIG, MID, NEXT, TANDEM, TWIN_A, TWIN_B, TINY = range(7)


def place(al):
    return al.a, al.strand, al.d


def ans(I=1000, R=2, B=0):
    return pc.answers(I, R, B)


def pair_of(name):
    return next((m1, m2) for n, m1, m2 in pc.table().pairs if n == name)


def find(genome_row, seq):
    """Where the (forward) sequence lies on its accession."""
    at = pc.table().rows[genome_row][1].find(seq)
    assert at >= 0
    return at


# ---- cases whose answer follows from how they were made ----------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
def test_hand_a_proper_pair_in_both_orientations(flip):
    """A fragment of 400 bases of `big`, two mates of 150: the forward mate at the fragment's start, the other 250 further on the
    other strand; both whole reads, score 150; FLAG 1 + 2 + 64 / 128, 16 on the reverse mate and 32 on its partner."""
    a = ans()
    name = "proper_F400_%d" % flip
    m1, m2 = pair_of(name)
    fwd, rev = (m2, m1) if flip else (m1, m2)
    at = find(BIG, fwd)
    assert find(BIG, ac.revcomp(rev)) == at + 250
    k1, k2 = a.kept[name]
    want_f, want_r = align.Aln(BIG, 0, at, 150, 0, 150, 0), align.Aln(BIG, 1, at + 250, 150, 0, 150, 0)
    assert (k1, k2) == (([want_r], [want_f]) if flip else ([want_f], [want_r])) and a.proper[name]
    recs = align.records([m1, m2], [k1, k2], [True])[0]
    flags = [int(r["flag_len"]) & 0xFFF for r in recs]
    assert flags == ([1 + 2 + 16 + 64, 1 + 2 + 32 + 128] if flip else [1 + 2 + 32 + 64, 1 + 2 + 16 + 128])
    assert [int(r["ref_new"]) >> 31 for r in recs] == [1, 0] and [int(r["flag_len"]) >> 12 for r in recs] == [150, 150]


def test_hand_the_insert_limit_is_inclusive():
    """F = I: v(r) - u(f) = F <= I, proper.  F = I + 1: both mates align as before, each alone: FLAG 1 without 2."""
    for I in (150, 212, 213, 214, 1000, 8192):
        a = pc.answers(I, 2, 8 if I == 213 else 0)
        for flip in (0, 1):
            assert a.proper["proper_F%d_%d" % (I, flip)] and not a.proper["proper_F%d_%d" % (I + 1, flip)], I
            k1, k2 = a.kept["proper_F%d_%d" % (I + 1, flip)]
            assert len(k1) == 1 and len(k2) == 1 and k1[0].score == k2[0].score == 150
            assert align.pair_flag(0, 0, k1[0], k2, False) == 1 + 64 + 16 * k1[0].strand + 32 * k2[0].strand


def test_hand_rescue_windows():
    """The anchor on strand 0 at d, L = L' = 150, I = 1000: the partner's place ends at most 1000 behind d, so d' <= d + 850, and it
    starts no earlier: d' >= d.  On strand 1 the mirror.  L' < L: the partner must end no earlier, d' >= d + L - L'.  The ends of
    the accession clip it; an empty range is none."""
    assert align.rescue_window(0, 500, 150, 150, 12000, 1000) == (500, 1350)
    assert align.rescue_window(1, 5000, 150, 150, 12000, 1000) == (4150, 5000)
    assert align.rescue_window(0, 500, 150, 100, 12000, 1000) == (550, 1400)
    assert align.rescue_window(0, 500, 100, 150, 12000, 1000) == (500, 1350)
    assert align.rescue_window(1, 5000, 150, 100, 12000, 1000) == (4150, 5000)
    assert align.rescue_window(1, 5000, 100, 150, 12000, 1000) == (4100, 4950)
    assert align.rescue_window(0, 11900, 150, 150, 12000, 1000) == (11900, 11999)
    assert align.rescue_window(1, 100, 150, 150, 12000, 1000) == (-149, 100)
    assert align.rescue_window(0, 0, 150, 150, 12000, 150) == (0, 0)
    assert align.rescue_window(0, 0, 150, 151, 12000, 150) is None and align.rescue_window(0, 0, 1024, 1024, 12000, 1000) is None
    assert align.rescue_window(0, 12100, 150, 150, 12000, 1000) is None


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("which", [1, 2])
def test_hand_a_mate_without_seeds_is_rescued_at_its_planted_place(which, flip):
    """Mate `which` has a substitution at every 12th base: no candidate, no alignment with R = 0; with R >= 1 the partner's one
    alignment is the anchor and the best diagonal of its window is the planted one: 13 substitutions, 150 - 13 - 4 * 13 = 85 at
    the least (the segment drops a mismatch next to an end: 89 here)."""
    name = "rescue%d_F400_%d" % (which, flip)
    m1, m2 = pair_of(name)
    for R in (0, 1, 2):
        a = ans(R=R)
        kept = a.kept[name]
        ncand, nacc, nref, nres, ntask = a.counts[name]
        good, bad = kept[2 - which], kept[which - 1]
        assert len(good) == 1 and good[0].score == 150
        if R == 0:
            assert bad == [] and not a.proper[name] and (nres, ntask) == (0, 0)
            assert align.pair_flag(2 - which, 0, good[0], bad, False) & 8
            continue
        assert a.proper[name] and (nacc, nres, ntask) == (2, 1, 1) and len(bad) == 1
        assert bad[0].strand == 1 - good[0].strand and abs(bad[0].d - good[0].d) == 250 and 85 <= bad[0].score <= 98


def test_hand_windows_of_exactly_1_63_64_and_65_diagonals():
    """Two mates of 150 and I = 150, 212, 213, 214: the window holds I - 149 diagonals and the planted place (F = I) is its last."""
    for I, B in ((150, 0), (212, 0), (213, 8), (214, 0)):
        a = pc.answers(I, 2, B)
        for flip in (0, 1):
            name = "rescue2_F%d_%d" % (I, flip)
            k1, k2 = a.kept[name]
            assert a.proper[name] and a.counts[name][3:] == (1, 1), (I, flip)
            lo, hi = align.rescue_window(k1[0].strand, k1[0].d, 150, 150, 12000, I)
            assert hi - lo + 1 == I - 149 and k2[0].d == (lo if flip else hi)
            assert not a.proper["rescue2_F%d_%d" % (I + 1, flip)]


def test_hand_mates_of_other_lengths_and_a_mate_inside_the_other():
    a = pc.answers(8192, 2, 0)
    for L1 in pc.LENGTHS:
        for L2 in pc.LENGTHS:
            name = "len_%d_%d" % (L1, L2)
            k1, k2 = a.kept[name]
            if min(L1, L2) >= 63:  # (a mate of 15 bases never reaches min_score 30; the others are all found, seeded or rescued)
                assert a.proper[name] and k1[0].a == k2[0].a == BIG, name
                (u1, v1), (u2, v2) = align.place_of(k1[0], L1), align.place_of(k2[0], L2)
                assert max(v1, v2) - min(u1, u2) == max(L1, L2) + (0 if (L1 + L2) % 2 else 137), name
            else:
                assert not a.proper[name]
    inside = a.kept["len_63_150"]  # F = 150: mate 1's 63 bases lie inside mate 2's 150
    (u1, v1), (u2, v2) = align.place_of(inside[0][0], 63), align.place_of(inside[1][0], 150)
    assert {inside[0][0].strand, inside[1][0].strand} == {0, 1} and min(u1, u2) == u2 and max(v1, v2) == v2


def test_hand_the_ends_of_an_accession():
    """A mate at the accession's first and last base, and hanging over either end by 12 bases: the window is clipped to
    [1 - L', n - 1], the rescued diagonal is negative on the left, and the columns outside the accession only reset the scan."""
    a, n = ans(), 5000
    assert place(a.kept["first_base"][0][0]) == (MID, 0, 0) and place(a.kept["last_base"][1][0]) == (MID, 1, n - 150)
    assert place(a.kept["first_base_flip"][1][0]) == (MID, 0, 0) and place(a.kept["last_base_flip"][0][0]) == (MID, 1, n - 150)
    left, right = a.kept["hang_left"][0][0], a.kept["hang_right"][1][0]
    assert place(left) == (MID, 0, -12) and left.b >= 12 and align.pos0_of(left) >= 0
    assert place(right) == (MID, 1, n - 138) and right.e <= 138
    for name in ("first_base", "last_base", "first_base_flip", "last_base_flip", "hang_left", "hang_right"):
        assert a.proper[name] and a.counts[name][3:] == (1, 1), name
    assert align.rescue_window(1, 230, 150, 150, n, 1000) == (-149, 230)  # (hang_left's: mate 2 is the anchor)


def test_hand_a_window_never_reaches_the_next_accession():
    """Mate 1 ends 50 bases before the end of `mid`; mate 2 lies on `next`, which follows it in memory, 150 bases on.  The window
    [4800, 4999] ends with the accession: there is a task, it finds nothing, and mate 2 has no record."""
    a = ans()
    for name, good in (("cross_next", 0), ("cross_prev", 0)):
        kept = a.kept[name]
        assert len(kept[good]) == 1 and kept[1 - good] == [] and not a.proper[name]
        assert a.counts[name][3:] == (0, 1), name
    assert align.rescue_window(0, 4800, 150, 150, 5000, 1000) == (4800, 4999)
    assert a.proper["tiny_window"] and place(a.kept["tiny_window"][1][0]) == (TINY, 1, 40)


def test_hand_equal_scores_in_a_tandem_repeat_resolve_to_the_smallest_diagonal():
    """Mate 2 lies inside 12 copies of a unit of 40 and cannot seed: diagonals 40 apart score alike as far as the repeat goes, and
    the smallest of the best wins.  tandem[700:850] is also tandem[620:770] (two units to the left, still inside the repeat that
    starts at 600), but not tandem[580:730]."""
    a = ans()
    t = pc.table()
    k1, k2 = a.kept["tandem_rescue"]
    o = align.revcomp_codes(refseq.codes_of(pair_of("tandem_rescue")[1]))
    scores = align.window_scores(o, t.ref.codes[TANDEM], 300, 1150, 4)
    assert place(k2[0]) == (TANDEM, 1, 620) and a.proper["tandem_rescue"]
    assert scores[620 - 300] == scores[660 - 300] == scores[700 - 300] == k2[0].score and scores.max() == k2[0].score
    assert scores[580 - 300] < k2[0].score
    k1, k2 = a.kept["tandem_rescue_flip"]  # the anchor on strand 1: the window lies to its left, the smallest is still the first
    assert place(k2[0]) == (TANDEM, 0, 620) and a.proper["tandem_rescue_flip"]


def test_hand_a_seeded_candidate_within_the_band_of_the_window_gives_no_task():
    """F = 1005: mate 2 seeds and is accepted 5 diagonals beyond the window's end.  At band 8 that is within B of it: no task.  At
    band 0 it is outside: two tasks (each mate's only alignment is an anchor), which find nothing.  F = 1040: tasks at either band."""
    assert pc.answers(1000, 2, 8).counts["seeded_near"][3:] == (0, 0)
    assert pc.answers(1000, 2, 0).counts["seeded_near"][3:] == (0, 2)
    assert pc.answers(1000, 2, 8).counts["seeded_far"][3:] == (0, 2)
    assert not pc.answers(1000, 2, 8).proper["seeded_near"]


def test_hand_two_anchors_that_rescue_one_diagonal_add_it_once():
    """Mate 1 lies inside the tandem repeat: accepted on several diagonals 40 apart with one score, the first two by (a, pos0) are
    the anchors at R = 2, and both windows hold mate 2's place: two tasks, one rescued candidate.  R = 1: one task."""
    a2, a1, a8 = ans(R=2), ans(R=1), pc.answers(8192, 8, 8)
    assert a2.counts["two_anchors"][3:] == (1, 2) and a1.counts["two_anchors"][3:] == (1, 1)
    assert a8.counts["two_anchors"][3] == 1 and a8.counts["two_anchors"][4] > 2
    assert a2.kept["two_anchors"] == a1.kept["two_anchors"] and a2.proper["two_anchors"]
    assert place(a2.kept["two_anchors"][1][0]) == (TANDEM, 1, 1150)


def test_hand_a_rescued_candidate_is_refined_with_the_band():
    """The unseedable mate has a deletion of 3 (an insertion of 2) 80 (70) bases in: without the band the rescued segment ends
    there; with band 8 it is refined like any accepted candidate and covers the read."""
    a0, a8 = ans(B=0), ans(B=8)
    for name, m, op in (("rescue_del", 1, "D" * 3), ("rescue_ins", 1, "I" * 2), ("rescue_del_flip", 0, "D" * 3)):
        short, full = a0.kept[name][m][0], a8.kept[name][m][0]
        assert isinstance(short, align.Aln) and short.e - short.b < 100 and a0.proper[name]
        assert isinstance(full, align.GapAln) and op in full.ops and full.e - full.b > 140 and full.score > short.score and a8.proper[name]
        assert a8.counts[name][2:4] == (1, 1)


def test_hand_unaligned_mates():
    a = ans()
    k1, k2 = a.kept["mate1_unaligned"]
    assert k1 == [] and len(k2) == 1 and not a.proper["mate1_unaligned"]
    recs = align.records(list(pair_of("mate1_unaligned")), [k1, k2], [False])[0]
    assert len(recs) == 1 and int(recs[0]["ref_new"]) >> 31 == 1 and int(recs[0]["flag_len"]) & 0xFFF == 1 + 8 + 16 + 128
    k1, k2 = a.kept["mate2_unaligned"]
    recs = align.records(list(pair_of("mate2_unaligned")), [k1, k2], [False])[0]
    assert len(recs) == 1 and int(recs[0]["flag_len"]) & 0xFFF == 1 + 8 + 64
    assert a.kept["both_unaligned"] == ([], []) and len(align.records(list(pair_of("both_unaligned")), [[], []], [False])[0]) == 0
    for name in ("mate2_short", "mate2_long", "mate1_empty"):  # a partner outside k <= L' <= 1024 is never sought
        assert a.counts[name][3:] == (0, 0) and not a.proper[name], name


def test_hand_the_pair_settles_a_multimapped_mate():
    """Mate 1 lies in the 400 bases twinA and twinB share, mate 2 on twinA alone.  Alone, mate 1 keeps both places; in the pair only
    the one with a concordant partner stays.  Both mates in the shared part: two proper pairs, the first by (a, pos0) the primary."""
    a = ans()
    t = pc.table()
    k1, k2 = a.kept["twin_settled"]
    assert [place(x) for x in k1] == [(TWIN_A, 0, 100)] and [place(x) for x in k2] == [(TWIN_A, 1, 500)]
    alone = align.align_read_gapped(pair_of("twin_settled")[0], t.index, t.ref, t.p, a.gp)[0]
    assert [place(x) for x in alone] == [(TWIN_A, 0, 100), (TWIN_B, 0, 100)]
    k1, k2 = a.kept["twin_both"]
    assert [place(x) for x in k1] == [(TWIN_A, 0, 50), (TWIN_B, 0, 50)] and [place(x) for x in k2] == [(TWIN_A, 1, 220), (TWIN_B, 1, 220)]
    flags = [int(r["flag_len"]) & 0xFFF for r in align.records(list(pair_of("twin_both")), [k1, k2], [True])[0]]
    assert flags == [1 + 2 + 32 + 64, 1 + 2 + 32 + 64 + 256, 1 + 2 + 16 + 128, 1 + 2 + 16 + 128 + 256]
    for name in ("two_accessions", "same_strand", "outward"):
        assert not a.proper[name] and all(len(k) == 1 for k in a.kept[name]), name


def test_hand_pair_choice_orders_and_secondaries():
    """Two lists on one accession.  The best sum wins; among equal sums the smallest place in the first list, then in the second.
    A secondary needs a concordant partner whose sum reaches sec_pct of the best; without a concordant pair each mate is alone."""
    A = align.Aln
    p, pp = align.params(), align.pair_params(1, 1000, 2)
    x0, x1, x2 = A(0, 0, 100, 150, 0, 150, 0), A(0, 0, 5000, 150, 0, 150, 0), A(0, 0, 9000, 100, 0, 100, 0)
    y0, y1, y2 = A(0, 1, 5300, 150, 0, 150, 0), A(0, 1, 400, 150, 0, 150, 0), A(0, 1, 9300, 40, 0, 40, 0)
    k1, k2, proper = align.select_pair([x0, x1, x2], 150, [y0, y1, y2], 150, p, pp)
    # C1 = [x0, x1, x2], C2 = [y1, y0, y2] by (score, a, pos0): (x0, y1) and (x1, y0) both sum to 300, x0 is the smaller place in C1
    assert proper and k1 == [x0, x1] and k2 == [y1, y0]  # x2 + y2 = 140 < 80 % of 300
    k1, k2, proper = align.select_pair([x0, x1, x2], 150, [y0, y1, y2], 150, p._replace(sec_pct=40), pp)
    assert k1 == [x0, x1, x2] and k2 == [y1, y0, y2]
    k1, k2, proper = align.select_pair([x0, x1, x2], 150, [y0, y1, y2], 150, p._replace(max_secondary=0), pp)
    assert k1 == [x0] and k2 == [y1] and proper
    k1, k2, proper = align.select_pair([x2], 150, [y0], 150, p, pp)  # no concordant pair: alone
    assert (k1, k2, proper) == ([x2], [y0], False)
    k1, k2, proper = align.select_pair([x1, x2], 150, [y0], 150, p._replace(sec_pct=0), pp)  # x2 has no concordant partner: dropped
    assert (k1, k2, proper) == ([x1], [y0], True)
    # the reverse mate in front of the forward one is no pair; the same place on both strands is (F = L)
    assert not align.concordant(A(0, 0, 500, 150, 0, 150, 0), 150, A(0, 1, 499, 150, 0, 150, 0), 150, 1000)
    assert align.concordant(A(0, 0, 500, 150, 0, 150, 0), 150, A(0, 1, 500, 150, 0, 150, 0), 150, 150)
    assert not align.concordant(A(0, 0, 500, 150, 0, 150, 0), 150, A(0, 1, 501, 150, 0, 150, 0), 150, 150)
    # clips count: [u, v) is the whole read's place
    assert align.place_of(A(0, 0, 500, 100, 20, 120, 0), 150) == (500, 650)
    assert align.place_of(align.GapAln(0, 1, 498, 90, 10, 140, 3, 510, 133, "M" * 60 + "DDD" + "M" * 70), 150) == (500, 653)


# ---- the definition against itself -------------------------------------------------------------------------------------------------
def test_window_scores_are_extends_scores():
    t = pc.table()
    for name, a, lo, hi in (("rescue2_F400_0", BIG, None, None), ("hang_left", MID, -149, 100), ("last_base", MID, 4700, 4999),
                            ("tandem_rescue", TANDEM, 500, 800), ("tiny_window", TINY, -149, 199)):
        for mate, strand in ((0, 0), (1, 1), (1, 0)):
            codes = refseq.codes_of(pair_of(name)[mate])
            o = align.revcomp_codes(codes) if strand else codes
            lo_, hi_ = (200, 700) if lo is None else (lo, hi)
            got = align.window_scores(o, t.ref.codes[a], lo_, hi_, 4)
            assert got.tolist() == [align.extend(o, t.ref.codes[a], d, 4)[0] for d in range(lo_, hi_ + 1)], (name, mate, strand)


def checked_select(real):
    seen = [0, 0]

    def select(accepted, p):
        kept = real(accepted, p)
        C = align.pair_list(accepted)
        view = [al for al in C if al.score * 100 >= C[0].score * p.sec_pct][:1 + p.max_secondary]
        assert kept == view, (accepted, kept, view)
        seen[0] += 1
        seen[1] += len(C) > len(kept)
        return kept
    return select, seen


def test_select_is_a_view_of_the_pair_list(monkeypatch):
    """select() equals pair_list() filtered by sec_pct and cut at 1 + max_secondary, on the accepted set of every read of
    tests/align_cases.py and tests/align_gap_cases.py: the tables are built again with a select() that checks it."""
    select, seen = checked_select(align.select)
    monkeypatch.setattr(align, "select", select)
    for k, w in ac.PARAMS:
        if (k, w) != (gc.K, gc.W):  # (that table's reads are among the gapped tables')
            ac.table.__wrapped__(k, w)
    for band in gc.BANDS:
        gc.table.__wrapped__(band)
    assert seen[0] > 500 and seen[1] > 10  # (and the filter and the cut did something)
    for I, R, B in pc.PARAM_SETS[:2]:  # the same on the pair table's accepted sets, the rescued among them
        pc.answers.__wrapped__(I, R, B)


@pytest.mark.parametrize("params", pc.PARAM_SETS, ids=lambda x: "I%d_R%d_B%d" % x)
def test_records_round_trip_through_the_pair_sam_text(params):
    """sam_lines() in pair mode, tokenised as stage C's host tokeniser does, gives exactly records(): the FLAG bits, the new-read
    bit on the pair's first record only (one QNAME for both mates), len(SEQ) on each mate's primary."""
    a, t = pc.answers(*params), pc.table()
    names = pc.all_names()
    seqs, alns, proper, stats, pstats = pc.batch_of(a, names)
    headers = [b"%s/%d extra" % (n.encode(), m + 1) for n in names for m in (0, 1)]
    sam = align.sam_lines(headers, seqs, None, t.names, t.lengths, alns, proper)
    recs = align.records(seqs, alns, proper)[0]
    got = map_and_profile.tokenise_sam(sam, {n: i for i, n in enumerate(t.names)})
    assert np.array_equal(got, recs) and len(recs) == stats.records > 150
    body = [ln.split(b"\t") for ln in sam if not ln.startswith(b"@")]
    assert all(f[6:9] == [b"*", b"0", b"0"] and f[4] == b"255" and not f[0].endswith((b"/1", b"/2")) for f in body)
    assert sum(1 for r in recs if int(r["ref_new"]) >> 31) == sum(1 for i in range(0, len(alns), 2) if alns[i] or alns[i + 1])
    assert stats.records == sum(len(x) for x in alns) and pstats.proper == sum(proper)


def test_with_pairs_off_the_old_functions_return_what_they_returned():
    """records() and sam_lines() without `proper` are the old ones; and a pair without a concordant pair and without rescue is its
    two mates, each aligned alone."""
    a, t = pc.answers(1000, 0, 8), pc.table()
    n = 0
    for name, m1, m2 in t.pairs:
        if a.proper[name]:
            continue
        for m, seq in enumerate((m1, m2)):
            assert a.kept[name][m] == align.align_read_gapped(seq, t.index, t.ref, t.p, a.gp)[0], name
            n += 1
    assert n > 100
    seqs, alns, _, _, _ = pc.batch_of(a, pc.all_names())
    old = align.records(seqs, alns)[0]
    assert all(int(r["flag_len"]) & 0xFFF & ~(16 | 256) == 0 for r in old)
    assert sum(1 for r in old if int(r["ref_new"]) >> 31) == sum(1 for x in alns if x)
    lines = align.sam_lines([b"r%d/1" % i for i in range(len(seqs))], seqs, None, t.names, t.lengths, alns)
    assert all(ln.split(b"\t")[0].endswith(b"/1") for ln in lines if not ln.startswith(b"@"))


def test_an_odd_number_of_reads_is_refused():
    t = pc.table()
    with pytest.raises(ValueError):
        align.align_reads_paired([b"ACGT" * 10] * 3, t.ref, t.p, align.gap_params(), align.pair_params(1), index=t.index)


# ---- the flags ---------------------------------------------------------------------------------------------------------------------
def test_pair_parameter_ranges():
    assert align.pair_params() == (0, 1000, 2) and align.pair_params("interleaved", 8192, 8) == (1, 8192, 8)
    assert align.pair_params("none", 1, 0) == (0, 1, 0)
    for bad, named in ((dict(max_insert=0), "--align_max_insert"), (dict(max_insert=8193), "--align_max_insert"),
                       (dict(rescue=-1), "--align_rescue"), (dict(rescue=9), "--align_rescue"), (dict(interleaved=2), "--align_pairs")):
        with pytest.raises(ValueError) as e:
            align.pair_params(**bad)
        assert named in str(e.value)


@pytest.mark.parametrize("tool,parse", [("metalign", metalign.metalign_parseargs), ("map_and_profile", map_and_profile.profile_parseargs)])
def test_the_flags_parse_with_their_defaults(tool, parse):
    a = parse(["reads.fq", "data"])
    assert (a.align_pairs, a.align_max_insert, a.align_rescue) == ("none", 1000, 2) and align_pair_params(a) == (0, 1000, 2)
    a = parse(["reads.fq", "data", "--aligner", "device", "--align_pairs", "interleaved", "--align_max_insert", "600", "--align_rescue", "0"])
    assert align_pair_params(a) == (1, 600, 0)
    with pytest.raises(SystemExit):
        parse(["reads.fq", "data", "--align_pairs", "by_name"])
    text = " ".join(cli.parser_for(tool).format_help().split())
    assert "BY POSITION" in text and "keeps no read names and compares none" in text


@pytest.mark.parametrize("tool,parse", [("metalign", metalign.metalign_parseargs), ("map_and_profile", map_and_profile.profile_parseargs)])
@pytest.mark.parametrize("extra,named", [(["--align_pairs", "interleaved", "--align_max_insert", "0"], "--align_max_insert"),
                                         (["--align_pairs", "interleaved", "--align_max_insert", "8193"], "--align_max_insert"),
                                         (["--align_pairs", "interleaved", "--align_rescue", "9"], "--align_rescue"),
                                         (["--align_rescue", "-1"], "--align_rescue"),
                                         (["--align_pairs", "interleaved", "--read_assignments", "x.tsv"], "--read_assignments")])
def test_check_flags_refuses_values_out_of_range(tool, parse, extra, named):
    argv = ["reads.fq", "data", "--aligner", "device"] + (["--db", "db.fna"] if tool == "map_and_profile" else []) + extra
    with pytest.raises(SystemExit) as e:
        check_flags(parse(argv))
    assert named in str(e.value)


@pytest.mark.parametrize("tool,parse", [("metalign", metalign.metalign_parseargs), ("map_and_profile", map_and_profile.profile_parseargs)])
def test_pairs_need_the_device_aligner(tool, parse):
    with pytest.raises(SystemExit) as e:
        check_flags(parse(["reads.fq", "data", "--align_pairs", "interleaved"]))
    assert "--aligner device" in str(e.value)
    check_flags(parse(["reads.fq", "data", "--aligner", "device", "--align_pairs", "interleaved"] + (["--db", "x"] if tool != "metalign" else [])))


def test_a_bam_of_reads_is_refused_as_paired_input(tmp_path):
    import gzip
    for name, data in (("plain.bam", b"BAM\x01" + b"\0" * 8), ("bgzf.bam", gzip.compress(b"BAM\x01" + b"\0" * 8))):
        (tmp_path / name).write_bytes(data)
        argv = [str(tmp_path / name), "data", "--aligner", "device", "--align_pairs", "interleaved"]
        with pytest.raises(SystemExit) as e:
            check_flags(metalign.metalign_parseargs(argv))
        assert "BAM" in str(e.value)
        check_flags(metalign.metalign_parseargs(argv[:4]))  # (single-end, a BAM of reads is fine)


def test_the_last_record_of_a_piece_is_found_on_the_host_text():
    fq = b"@a x\nACGT\n+\nIIII\n@b\nAC\n+\n@I\n@c\nA\n+\n@\n"
    assert map_and_profile._last_record_start(fq, len(fq), "fastq") == fq.index(b"@c")
    assert map_and_profile._last_record_start(fq, fq.index(b"@c"), "fastq") == fq.index(b"@b")
    assert map_and_profile._last_record_start(fq, fq.index(b"@b"), "fastq") == 0
    assert map_and_profile._last_record_start(fq.replace(b"\n", b"\r\n"), len(fq) + 12, "fastq") == fq.replace(b"\n", b"\r\n").index(b"@c")
    fa = b">a x\nACGT\nAC>GT\n>b\nAC\n\n>c\nA\n"
    assert map_and_profile._last_record_start(fa, len(fa), "fasta_ml") == fa.index(b">c")
    assert map_and_profile._last_record_start(fa, fa.index(b">c"), "fasta_ml") == fa.index(b">b")
    assert map_and_profile._last_record_start(fa, fa.index(b">b"), "fasta_ml") == 0


# ---- mg_align_pair_core.h under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pair_check") / "host_align_pair_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_align_pair_check.cpp")])
    return out


def fields(al, L=None):
    f = [al.a, al.strand, al.score, align.pos0_of(al), align.span_of(al), al.b, al.e]
    return f + ([L] if L is not None else [])


def choice_line(acc1, L1, acc2, L2, p, pp):
    """A P case and what the definition says of it."""
    C1, C2 = align.pair_list(acc1), align.pair_list(acc2)
    case = ["P", pp.max_insert, p.sec_pct, p.max_secondary, len(C1), L1, len(C2), L2] + [v for al in C1 + C2 for v in fields(al)]
    k1, k2, proper = align.select_pair(acc1, L1, acc2, L2, p, pp)
    best = max((x.score + y.score for x in C1 for y in C2 if align.concordant(x, L1, y, L2, pp.max_insert)), default=0)
    want = "P %d %d" % (proper, best)
    for m, (kept, C, partner) in enumerate(((k1, C1, k2), (k2, C2, k1))):
        want += " |" + "".join(" %d:%d" % (C.index(al), align.pair_flag(m, t, al, partner, proper)) for t, al in enumerate(kept))
    return case, want


def test_core_header_against_the_definition(exe, tmp_path):
    """Windows at every clipping, concordance of every two alignments of the pair table's answers, and the pair choice on every
    pair's accepted sets (the rescued and refined among them) under other sec_pct and max_secondary, against the definition."""
    import random
    rng = random.Random(9)
    cases, want = [], []
    for _ in range(3000):
        s, L, Lp = rng.randrange(2), rng.choice([15, 63, 150, 151, 1024]), rng.choice([15, 64, 150, 1024])
        n, I = rng.choice([1, 200, 5000, 2 ** 32 - 1]), rng.choice([1, 150, 151, 1000, 8192])
        d = rng.choice([-1009, -1, 0, 1, n // 2, n - 151, n - 1])
        cases.append(["W", s, d, L, Lp, n, I])
        win = align.rescue_window(s, d, L, Lp, n, I)
        want.append("W 1 %d %d" % win if win else None)
    t = pc.table()
    for params in ((1000, 2, 8), (8192, 8, 8), (214, 2, 0)):
        a = pc.answers(*params)
        flat = [(al, len(seq)) for name, m1, m2 in t.pairs for kept, seq in zip(a.kept[name], (m1, m2)) for al in kept]
        for _ in range(3000):
            (x, Lx), (y, Ly) = rng.choice(flat), rng.choice(flat)
            cases.append(["C"] + fields(x, Lx) + fields(y, Ly) + [a.pp.max_insert])
            want.append("C %d" % align.concordant(x, Lx, y, Ly, a.pp.max_insert))
        for name, m1, m2 in t.pairs:
            codes = [refseq.codes_of(m1), refseq.codes_of(m2)]
            acc = [align.accepted_of(c, t.index, t.ref, t.p)[1] for c in codes]
            added, _ = align.rescue_pair(codes, acc, t.ref, t.p, a.gp, a.pp)
            acc = [acc[0] + added[0], acc[1] + added[1]]
            for change in (dict(), dict(sec_pct=0, max_secondary=15), dict(max_secondary=0), dict(sec_pct=100, max_secondary=1)):
                case, w = choice_line(acc[0], len(m1), acc[1], len(m2), t.p._replace(**change), a.pp)
                cases.append(case)
                want.append(w)
    A = align.Aln  # lists of sixteen, ties and overlaps: made-up alignments
    for _ in range(300):
        lists = [[A(rng.randrange(2), rng.randrange(2), rng.randrange(-100, 3000), rng.choice([60, 100, 150]), 0, 150, 0)
                  for _ in range(rng.randrange(0, 40))] for _ in (0, 1)]
        lists = [[al._replace(b=max(0, -al.d)) for al in ls] for ls in lists]
        case, w = choice_line(lists[0], 150, lists[1], 150, align.params(sec_pct=rng.choice([0, 50, 80]), max_secondary=rng.choice([0, 5, 15])),
                              align.pair_params(1, rng.choice([300, 1000, 8192]), 2))
        cases.append(case)
        want.append(w)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(v) for v in c) for c in cases) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d cases" % len(cases) and len(lines) == len(cases) + 1
    nproper = 0
    for c, got, w in zip(cases, lines, want):
        if w is None:
            assert got.startswith("W 0 "), (c, got)
        else:
            assert got == w, (c, got, w)
        nproper += got.startswith("P 1")
    assert nproper > 500 and sum(1 for w in want if w and w.startswith("C 1")) > 100


# ---- the rescue property -----------------------------------------------------------------------------------------------------------
def test_unseedable_mates_are_rescued_and_only_by_rescue():
    """300 pairs from a genome of 20 000 bases, fragments of 300 to 600; mate 2 has a substitution at every 12th base, so no 15-mer of
    it survives, while its planted diagonal scores about 7 per 12 columns.  Every parameter at its default but the pairs: with R = 2
    at least 295 of 300 pairs come out proper with both primaries at their planted places, with R = 0 none.  Measured: 300 and 0."""
    names, lengths, fasta, ref, seqs, truth = pc.property_inputs()
    p, gp = align.params(), align.gap_params()
    index = align.build_index(ref, p.k, p.w)
    assert all(align.candidates(refseq.codes_of(s), index, p) == set() for s in seqs[1::2])
    found = {}
    for R in (2, 0):
        alns, proper, stats, pstats = align.align_reads_paired(seqs, ref, p, gp, align.pair_params(1, 1000, R), index=index)
        found[R] = sum(pc.planted(alns[2 * i], alns[2 * i + 1], proper[i], truth[i]) for i in range(300))
        print("R = %d: %d of 300 planted pairs, %s, %s" % (R, found[R], stats, pstats))
        assert R or pstats.rescued == 0
    assert found[2] >= 295 and found[0] == 0
    assert (found[2], found[0]) == (300, 0)


# ---- what a pair does to the profile -----------------------------------------------------------------------------------------------
def test_a_pair_counts_as_one_read_unique_to_the_taxon_both_mates_hit():
    """Mate 1 hits twinA and twinB equally, mate 2 twinA alone.  Through stage C's host path (assignments.read_assignments: the
    reference's read loop) the pair's SAM text is ONE read, unique to twinA's taxon; the same two reads aligned without pairs are one
    multimapped read and one unique read.  The first read loses its first line to the read loop's phantom boundary (it has a second), and the last is never decided."""
    t = pc.table()
    a = ans()
    head, twin, tail = pair_of("twin_both"), pair_of("twin_settled"), pair_of("proper_F400_1")  # (head: two lines per mate)
    seqs = list(head) + list(twin) + list(tail)
    headers = [b"head/1", b"head/2", b"twin/1", b"twin/2", b"tail/1", b"tail/2"]
    acc2info = {n: [ln, "tax_" + n, "n", "l"] for n, ln in zip(t.names, t.lengths)}
    alns, proper, stats, pstats = align.align_reads_paired(seqs, t.ref, t.p, a.gp, a.pp, index=t.index)
    assert proper == [True, True, True] and [len(x) for x in alns] == [2, 2, 1, 1, 1, 1]
    sam = align.sam_lines(headers, seqs, None, t.names, t.lengths, alns, proper)
    rows = list(assignments.read_assignments(sam, acc2info, 0.5))
    assert rows[1:] == [("twin", "U", ["tax_twinA"], 300), ("tail", "N", [], -1)] and rows[0][0] == "head"
    single = align.align_reads_gapped(seqs, t.ref, t.p, a.gp, index=t.index)[0]
    assert [len(x) for x in single] == [2, 2, 2, 1, 1, 1]
    sam = align.sam_lines(headers, seqs, None, t.names, t.lengths, single)
    rows = list(assignments.read_assignments(sam, acc2info, 0.5))
    assert rows[2:4] == [("twin/1", "M", ["tax_twinA", "tax_twinB"], 150), ("twin/2", "U", ["tax_twinA"], 150)] and len(rows) == 6
