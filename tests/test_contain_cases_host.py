"""The case table of tests/contain_cases.py reaches what it claims (so that a later edit, or a retuned constant in mg_contain.hip,
cannot move the kernels away from the cases silently), and its definition is the oracle's.  No GPU."""
import os
import re

import numpy as np
import pytest

import contain_cases as cc

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metalign_amd", "csrc", "mg_contain.hip")
ALL = [(fam, c) for fam, make in cc.FAMILIES.items() for c in make()]


def _geo(family):
    return {c.name: cc.case_geometry(c) for c in cc.FAMILIES[family]()}


# ---------------------------------------------------------------- the model's constants are the source's
def test_the_model_copies_the_constants_of_the_source():
    with open(SRC) as f:
        text = f.read()

    def one(pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return found[0]

    assert int(one(r"constexpr int kCT = (\d+);")) == cc.KCT
    assert int(one(r"constexpr int kCTile = (\d+) \* kCT;")) * cc.KCT == cc.KCTILE
    assert int(one(r"constexpr uint32_t kCCap = (\d+);")) == cc.KCCAP
    one(r"const bool staged = len < kCCap;")                      # 2047 is staged, 2048 is not
    one(r"while \(pow2 <= len\) pow2 <<= 1;")                     # the padded length is the smallest power of two ABOVE len
    per, cap = one(r"while \(\(1ull << lb\) < \(n \+ (\d+)\) / (\d+) && lb < (\d+)\) \+\+lb;")[1:]
    assert (int(per), int(cap)) == (cc.PER_BUCKET, cc.LB_MAX)
    assert int(one(r"while \(\(1ull << lb\) < \(n \+ (\d+)\) / \d+ && lb < \d+\) \+\+lb;")) == cc.PER_BUCKET - 1
    one(r"sk->index_shift = bits - lb;")
    one(r"hi = idx\[\(top >> shift\) \+ 1\];")
    # the copies rule, once per launcher (containment, by identity, count step)
    rules = re.findall(r"while \(copies < (\d+) && \(uint64_t\)copies \* 2 \* [\w>-]+ <= (\d+)\) copies \*= 2;", text)
    assert rules == [(str(cc.COPIES_MAX), str(cc.COPIES_BUDGET))] * 3
    # a rank's run of a count list
    one(re.escape("const uint64_t lo = nc / W * r + (nc % W) * r / W, hi = r + 1 == W ? nc : nc / W * (r + 1) + (nc % W) * (r + 1) / W;"))
    # the tile's last pair is picked from register il / kCT of thread il % kCT
    one(re.escape("for (int j = 1; j < kPer; ++j) v = (il / kCT) == (uint64_t)j ? h[j] : v;"))


# ---------------------------------------------------------------- the definition is the oracle's
@pytest.mark.parametrize("family", list(cc.FAMILIES))
def test_the_definition_equals_the_oracle(oracle_lib, family):
    for c in cc.FAMILIES[family]():
        hashes, offsets = cc.genome_major(c)
        qh, qc, trunc = c.q_hashes, c.q_counts, c.truncated
        if trunc and (len(qh) == 0 or c.bound != int(qh[-1])):
            # the oracle's bound is the sketch's last hash: an entry AT the bound that no ci reaches puts it there
            assert len(qh) == 0 or c.bound > int(qh[-1])
            qh, qc = np.append(qh, np.uint64(c.bound)), np.append(qc, np.uint32(0))
        for ci in (1, 2, 3):
            hits, sizes = cc.want(c, ci)
            ohits, osizes = oracle_lib.containment(qh, qc, trunc, ci, hashes if len(hashes) else np.zeros(1, np.uint64), offsets)
            assert np.array_equal(hits, ohits) and np.array_equal(sizes, osizes), (c.name, ci)
            assert hits.dtype == np.uint32 and sizes.dtype == np.uint32 and len(hits) == len(sizes) == c.ngenomes


def test_every_case_is_valid_input_within_the_size_limits():
    names = set()
    for fam, c in ALL:
        assert (fam, c.name) not in names
        names.add((fam, c.name))
        assert len(c.feed_hashes) <= 200000 and len(c.pair_hash) <= 100000 and 1 <= c.ngenomes <= 33000, c.name
        assert np.all(c.q_hashes[:-1] < c.q_hashes[1:]) and int(c.q_counts.max(initial=0)) <= 3
        assert int(c.feed_hashes.max(initial=0)) <= cc.TOP and int(c.pair_hash.max(initial=0)) <= cc.TOP
        assert np.all(c.pair_hash[:-1] <= c.pair_hash[1:]) and int(c.pair_gen.max(initial=0)) < c.ngenomes
        assert np.array_equal(c.gsize, np.bincount(c.pair_gen.astype(np.int64), minlength=c.ngenomes))
        # the sketch the library will make of the feed: its s smallest, truncated when something was cut
        assert np.array_equal(c.q_hashes, np.sort(c.feed_hashes)[:len(c.q_hashes)])
        assert len(c.q_hashes) == (c.s if c.s else len(c.feed_hashes)) and (c.set_bound is not None or c.truncated == (c.s > 0))
        if c.truncated and len(c.q_hashes):
            assert c.bound >= int(c.q_hashes[-1])
    for group in cc.MULTI.values():
        assert 2 <= len(group) <= 4 and len(set(group)) == len(group)
        for fam, name in group:
            cc.case(fam, name)


# ---------------------------------------------------------------- every family reaches its edges
def test_run_lengths_reach_every_length_on_both_paths():
    (c,) = cc.run_lengths()
    geo = cc.case_geometry(c)
    assert (geo.shift, geo.buckets) == (cc.RUN_SHIFT, 2048) and int(c.q_hashes[-1]).bit_length() == 64
    assert [t.run_len for t in geo.tiles] == cc.RUN_LENGTHS and all(t.t1 - t.t0 == cc.KCTILE for t in geo.tiles)
    by = {t.run_len: t for t in geo.tiles}
    assert by[2047].staged and by[2047].pow2 == cc.KCCAP and not by[2048].staged and not by[2049].staged and not by[5000].staged
    assert (by[1023].pow2, by[1024].pow2, by[1025].pow2) == (1024, 2048, 2048)  # the padding doubles between 1023 and 1024
    assert (by[255].pow2, by[256].pow2, by[0].pow2, by[1].pow2, by[2].pow2) == (256, 512, 1, 2, 4)
    for t, length in zip(geo.tiles, cc.RUN_LENGTHS):
        lo, hi = cc.run_span(geo.tiles.index(t), length)
        ph = c.pair_hash[t.t0:t.t1]
        assert lo < t.h_first and t.h_last < hi and (t.h_first >> geo.shift) == lo >> geo.shift and (t.h_last >> geo.shift) == hi >> geo.shift
        run, cnt = c.q_hashes[t.lo:t.hi], c.q_counts[t.lo:t.hi]
        assert np.all((run > np.uint64(lo)) & (run < np.uint64(hi)))
        if not length:
            continue
        # matches on the first and the last entry of the run at every ci; non-matches at hash +- 1 of a present hash
        assert cnt[0] == 3 and cnt[-1] == 3 and run[0] in ph and run[-1] in ph
        present = np.isin(ph, run)
        assert present.sum() >= 4
        assert np.isin(ph + np.uint64(1), run).sum() >= min(length, 100) and np.isin(ph - np.uint64(1), run).sum() >= min(length, 100)
        assert not np.isin(ph[np.isin(ph + np.uint64(1), run)], run).any()
        if length >= 255:  # counts on either side of every ci, among the entries that pairs look up
            looked = cnt[np.isin(run, ph)]
            assert set(looked.tolist()) == {0, 1, 2, 3}
    for ci in (1, 2, 3):
        hits, _ = cc.want(c, ci)
        assert hits.sum() > 1000 and (ci == 1 or hits.sum() < cc.want(c, ci - 1)[0].sum())


def test_tile_edges_take_every_pick_of_the_last_pair():
    cases = {c.name: c for c in cc.tile_edges()}
    geo = _geo("tile_edges")
    assert [len(cases["npairs=%d" % n].pair_hash) for n in cc.TILE_NPAIRS] == cc.TILE_NPAIRS
    assert set(cc.TILE_NPAIRS) >= {1, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097}
    last = [geo["npairs=%d" % n].tiles[-1] for n in cc.TILE_NPAIRS]
    assert {t.slot for t in last} == set(range(8))                            # every branch of the s_edge[1] pick
    assert {(t.t1 - 1 - t.t0) % cc.KCT for t in last} >= {0, 254, 255}        # ... by the first and the last thread
    assert {len(geo["npairs=%d" % n].tiles) for n in cc.TILE_NPAIRS} == {1, 2, 3}
    for n in cc.TILE_NPAIRS:
        c = cases["npairs=%d" % n]
        at = np.searchsorted(c.q_hashes, c.pair_hash[-1])
        assert c.q_hashes[at] == c.pair_hash[-1] and c.q_counts[at] == 3      # the last pair is a match ...
        g = int(c.pair_gen[-1])
        assert all(cc.want(c, ci)[0][g] == 1 for ci in (1, 2, 3)) and c.gsize[g] == 1  # ... and its genome's only pair
        # a last hash picked from an EARLIER register cuts the run short of entries that match
        t = geo[c.name].tiles[-1]
        if t.slot:
            early = int(c.pair_hash[t.t0 + (t.t1 - 1 - t.t0) % cc.KCT])
            cut = int(np.searchsorted(c.q_hashes >> np.uint64(geo[c.name].shift), np.uint64((early >> geo[c.name].shift) + 1)))
            assert cut < t.hi and np.isin(c.q_hashes[cut:t.hi], c.pair_hash[t.t0:t.t1]).any()
        assert set(np.flatnonzero(c.gsize == 0).tolist()) >= set(cc.EMPTY_GENOMES)  # empty genomes first, in a run, last
        if n >= 4:
            pairs = np.stack([c.pair_hash, c.pair_gen.astype(np.uint64)])
            assert len(np.unique(pairs, axis=1)[0]) < n                       # a pair listed twice
    assert cases["no pairs"].ngenomes == 4 and geo["no pairs"].tiles == []
    # one hash in 5000 genomes: whole tiles with h_first == h_last, the hash present, absent, present below ci
    for kind, count in (("present", 3), ("absent", 0), ("present below ci", 1)):
        c = cases["one hash in %d genomes, %s" % (cc.SHARED, kind)]
        whole = [t for t in geo[c.name].tiles if t.h_first == t.h_last]
        assert whole and all(t.t1 - t.t0 == cc.KCTILE for t in whole) and c.ngenomes >= 5000
        h = np.uint64(whole[0].h_first)
        assert (c.pair_hash == h).sum() == cc.SHARED
        assert (c.q_counts[c.q_hashes == h].tolist() or [0]) == [count]
        shared = np.bincount(c.pair_gen[c.pair_hash == h], minlength=c.ngenomes)
        for ci in (1, 2, 3):
            assert (cc.want(c, ci)[0] >= shared).all() == (count >= ci)


def test_hash_edges_reach_the_ends_of_the_hash_range_and_of_the_index():
    cases = {c.name: c for c in cc.hash_edges()}
    geo = _geo("hash_edges")
    assert [len(cases["n=%d" % n].q_hashes) for n in cc.SMALL_N] == cc.SMALL_N == [1, 2, 7, 8, 9, 16, 17]
    assert {geo["n=%d" % n].buckets for n in cc.SMALL_N} == {2, 4} and geo["n=8"].buckets == 2 and geo["n=17"].buckets == 4
    for n in cc.SMALL_N:
        c = cases["n=%d" % n]
        assert int(c.q_hashes[-1]) == cc.TOP == 2 ** 64 - 2 and int(c.q_hashes[-1]).bit_length() == 64
        assert n < 2 or int(c.q_hashes[0]) == 0
        assert n < 7 or {1 << 63, (1 << 63) - 1} <= set(c.q_hashes.tolist())
        table = set(c.pair_hash.tolist())
        for h in c.q_hashes.tolist():
            assert {max(h - 1, 0), h, min(h + 1, cc.TOP)} <= table
        shift = geo[c.name].shift
        assert all({b << shift, (b << shift) - 1} <= table for b in range(1, geo[c.name].buckets))
    assert geo["n=1, hash 0"].shift == 0 and cases["n=1, hash 0"].q_hashes.tolist() == [0]
    assert cases["n=1, hash 2^63"].q_hashes.tolist() == [1 << 63] and cases["n=2, hashes 0 and 1"].q_hashes.tolist() == [0, 1]
    # the table entirely below q[0], entirely above q_last
    c = cases["table below the sketch"]
    assert int(c.pair_hash[-1]) < int(c.q_hashes[0]) and all(t.run_len == 0 for t in geo[c.name].tiles) and len(geo[c.name].tiles) == 2
    c = cases["table above the sketch"]
    assert int(c.pair_hash[0]) > int(c.q_hashes[-1]) and all((t.lo, t.hi) == (0, 0) for t in geo[c.name].tiles)
    assert (int(c.pair_hash[0]) >> geo[c.name].shift) > geo[c.name].buckets  # (its bucket number lies behind the index)
    # a tile straddles q_last, on both paths; table hashes equal q_last and q_last + 1
    for kind, staged in (("staged", True), ("per pair", False)):
        c = cases["a tile straddles the last hash, %s" % kind]
        t, q_last = geo[c.name].tiles[0], int(c.q_hashes[-1])
        assert t.h_first <= q_last < t.h_last and t.staged == staged and t.run_len > 400 and t.hi == len(c.q_hashes)
        assert q_last.bit_length() == 40 and {q_last, q_last + 1} <= set(c.pair_hash[t.t0:t.t1].tolist())
        assert (t.h_last >> geo[c.name].shift) > geo[c.name].buckets
    # hashes on bucket borders, in the sketch and as the first / last pair of a staged and of an unstaged tile
    c, g = cases["bucket borders"], geo["bucket borders"]
    width = 1 << g.shift
    q = set(c.q_hashes.tolist())
    assert g.buckets == 1024 and [t.staged for t in g.tiles] == [True, False, True]
    assert all({b * width, b * width - 1} <= q for b in range(1, g.buckets))
    for t in g.tiles:
        assert t.h_first % width == 0 and ((t.h_last + 1) % width == 0 or t.h_last == cc.TOP) and t.h_first in q and t.h_last in q
    table = set(c.pair_hash.tolist())
    assert sum(1 for b in range(1, g.buckets) if b * width in table) > 500 and sum(1 for b in range(1, g.buckets) if b * width - 1 in table) > 500
    assert sum(1 for b in range(1, g.buckets) if b * width + 1 in table and b * width + 1 not in q) > 200
    assert g.tiles[-1].h_last == cc.TOP and g.tiles[-1].t1 - g.tiles[-1].t0 == 300
    # one thread of k_build_index fills thousands of buckets
    c, g = cases["a gap of empty buckets"], geo["a gap of empty buckets"]
    stores = cc.index_stores(c.q_hashes, g.shift)
    assert g.buckets == 4096 and stores.max() > 3900 and stores.sum() == (int(c.q_hashes[-1]) >> g.shift) + 2
    runs = [(t.lo, t.hi) for t in g.tiles]
    assert runs[1] == (10000, 10000) and runs[0][1] <= 10000 and runs[2][0] == 10000 and runs[3][1] == 20000  # (a tile inside the gap)
    assert all(cc.want(c, 1)[0].sum() > 500 for c in (cases["bucket borders"], cases["a gap of empty buckets"]))


def test_bounds_cut_the_table_where_they_claim():
    cases = {c.name: c for c in cc.bounds()}
    cut = {name: cc.npairs_taking_part(c) for name, c in cases.items()}
    c = cases["s: the bound is the hash whose run crosses a tile boundary"]
    a, b = cc.CROSS
    assert a < cc.KCTILE < b - 1 and cut[c.name] == b and len(set(c.pair_hash[a:b].tolist())) == 1 and int(c.pair_hash[a]) == c.bound
    assert c.s > 0 and c.truncated and cc.case_geometry(c).tiles[-1].h_first == cc.case_geometry(c).tiles[-1].h_last == c.bound
    assert cut["set_bound: the crossing hash, the sketch ends below it"] == b
    for name in ("s: the bound lies below the first pair", "set_bound: below the first pair"):
        assert cut[name] == 0 and cases[name].truncated and cc.case_geometry(cases[name]).tiles == []
        hits, sizes = cc.want(cases[name], 1)
        assert not hits.any() and not sizes.any() and cases[name].gsize.all()
    assert cut["s: the bound is the last pair of the second tile"] == 2 * cc.KCTILE
    assert cut["s: the bound is the table's last hash"] == 5000 == cut["set_bound: above the table"] == cut["set_bound: not truncated"]
    c = cases["set_bound: between two hashes"]
    assert cut[c.name] == 3001 and c.bound not in set(c.pair_hash.tolist()) and int(c.q_hashes[-1]) < c.bound
    c = cases["set_bound: an empty sketch"]
    assert len(c.q_hashes) == 0 and c.truncated and cut[c.name] == 2501 and cc.want(c, 1)[1].sum() == 2501
    c = cases["set_bound: not truncated"]
    assert not c.truncated and c.set_bound[1] < int(c.pair_hash[-1]) and np.array_equal(cc.want(c, 2)[1], c.gsize)
    assert {bool(c.set_bound) for c in cases.values()} == {False, True} and sum(c.s > 0 for c in cases.values()) == 4
    # a cut that is off by one pair changes the sizes
    for c in cases.values():
        if c.truncated and 0 < cut[c.name] < 5000:
            assert cc.want(c, 1)[1].sum() == cut[c.name] and int(c.pair_hash[cut[c.name] - 1]) <= c.bound < int(c.pair_hash[cut[c.name]])


def test_copies_cross_the_steps_of_the_rule():
    cases = cc.copies_cases()
    assert [c.ngenomes for c in cases] == cc.COPIES_GENOMES and set(cc.COPIES_GENOMES) >= {1, 2, 512, 513, 32768, 32769}
    assert [cc.copies(g) for g in cc.COPIES_GENOMES] == [64, 64, 64, 64, 64, 32, 2, 1]
    assert [cc.copies(g) for g in (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385)] == [32, 16, 16, 8, 8, 4, 4, 2]
    for c in cases:
        for ci in (1, 2, 3):
            hits, _ = cc.want(c, ci)
            assert hits[c.ngenomes - 1] >= cc.HOT // 4 and hits[c.ngenomes // 2] >= cc.HOT // 4  # thousands of hits on one genome
        assert cc.want(c, 1)[0][c.ngenomes - 1] >= cc.HOT and len(cc.case_geometry(c).tiles) == 5
    # the largest table of a multi call decides for all of them
    sizes = {name: [cc.case(f, n).ngenomes for f, n in group] for name, group in cc.MULTI.items()}
    assert cc.copies(max(sizes["zero tiles first, one counter copy"])) == 1 and min(sizes["zero tiles first, one counter copy"]) == 4
    assert {cc.copies(max(s)) for s in sizes.values()} == {1, 8, 64}


def test_multi_groups_hold_a_neighbour_without_tiles_in_every_place():
    where = set()
    for name, group in cc.MULTI.items():
        cases = [cc.case(f, n) for f, n in group]
        for i, c in enumerate(cases):
            if cc.npairs_taking_part(c) == 0:
                where.add("first" if i == 0 else "last" if i == len(cases) - 1 else "middle")
    assert where == {"first", "middle", "last"}
    mixed = [cc.case(f, n) for f, n in cc.MULTI["truncated beside untruncated"]]
    assert {c.truncated for c in mixed} == {False, True}
    # tiles of a later k begin where a ragged tile of the one before ended
    ragged = [cc.npairs_taking_part(cc.case(f, n)) % cc.KCTILE != 0 for group in cc.MULTI.values() for f, n in group[:-1]]
    assert any(ragged) and not all(ragged)


# ---------------------------------------------------------------- the reference pipeline's table
def test_refpipe_definitions_equal_the_oracle(oracle_lib):
    for rc in cc.refpipe():
        table = cc.oracle_table(rc)
        for ci in (1, 2, 3):
            matched = cc.matched_by_hash(rc.q_hashes, rc.q_counts, ci, rc.pair_hash)
            assert np.array_equal(matched, oracle_lib.refpipe_matched(rc.q_hashes, rc.q_counts, ci, rc.pair_hash).astype(bool))
            hits, sizes = cc.refpipe_expected(rc, matched)
            ohits, osizes = oracle_lib.refpipe_containment(rc.q_hashes, rc.q_counts, ci, table)
            assert np.array_equal(hits, ohits) and np.array_equal(sizes, osizes), (rc.name, ci)
            for t in rc.small:
                assert np.array_equal(cc.mark_words(cc.marks_of(matched, t)), oracle_lib.refpipe_mark_words(matched, t))
            for cs in (0, 3):
                counts = cc.counters(rc, ci, cs)
                by_id = cc.matched_by_identity(counts, rc.head, ci, cs)
                # the oracle takes the per-pair counters: the head's, saturated
                per_pair = counts[rc.head.astype(np.int64)] if len(counts) else counts
                per_pair = np.minimum(per_pair, cs) if cs else per_pair
                hits, sizes = cc.refpipe_expected(rc, by_id)
                ohits, osizes = oracle_lib.refpipe_containment_counts(per_pair, ci, table)
                assert np.array_equal(hits, ohits) and np.array_equal(sizes, osizes), (rc.name, ci, cs)


def test_refpipe_cases_reach_their_edges():
    cases = {rc.name: rc for rc in cc.refpipe()}
    assert [[len(t["cid"]) for t in rc.small] for rc in cases.values()] == [[2047, 2048, 2049], [4096, 4100], [1], [0, 0]]
    starts = set()
    for rc in cases.values():
        assert len(rc.pair_hash) <= 100000 and len(rc.ks) == len(rc.small) + 1 and 15 <= rc.ks[-1] <= 64
        tile0 = 0
        for t in rc.small:
            npre = t["nprefix"]
            # the upload's own checks: numbers in range, the list ascending and derived from pa by the table's rule
            assert np.all(t["pa"] < npre) and np.all((t["pb"] < npre) | (t["pb"] == cc.NONE)) and np.all(t["cid"][:-1] <= t["cid"][1:])
            cid, cgen, gs = cc.count_list(t["pa"], rc.pair_gen, rc.ngenomes)
            assert np.array_equal(cid, t["cid"]) and np.array_equal(cgen, t["cgen"]) and np.array_equal(gs, t["gsize"])
            assert len(set(zip(t["cid"].tolist(), t["cgen"].tolist()))) == len(t["cid"])
            if tile0:
                starts.add(before % cc.KCTILE == 0)
            tile0, before = tile0 + -(-len(t["cid"]) // cc.KCTILE), len(t["cid"])
            if len(rc.pair_hash) < 2000:
                continue
            edge = {0, 31, 32, 63, npre - 1}
            assert edge <= set(t["pa"].tolist()) and edge <= set(t["pb"].tolist()) and edge <= set(t["cid"].tolist())
            assert (t["pb"] == cc.NONE).sum() > 100 and (t["pb"] == t["pa"]).sum() > 100 and (t["pb"] == 40).sum() > 100
            for ci in (1, 2, 3):
                matched = cc.matched_by_hash(rc.q_hashes, rc.q_counts, ci, rc.pair_hash)
                marks = cc.marks_of(matched, t)
                assert 0 < matched.sum() < len(matched) // 4 and marks[40]
                listed = marks[t["cid"].astype(np.int64)]  # marked and unmarked entries of the list side by side: a shifted bit changes the counts
                assert min(listed.sum(), (~listed).sum()) >= 50 and (listed[1:] != listed[:-1]).sum() >= 50
                words = cc.mark_words(marks)
                assert len(words) == (npre + 31) // 32 and all(bool(words[p >> 5] >> (p & 31) & 1) == bool(marks[p]) for p in edge)
    assert starts == {False, True}  # a later k's list begins behind a ragged and behind a whole last tile of the list before it
    big = cases["count lists of 2047, 2048, 2049"]
    for world in cc.REFPIPE_WORLDS:
        for t in big.small:
            runs = [cc.count_share(len(t["cid"]), r, world) for r in range(world)]
            assert runs[0][0] == 0 and runs[-1][1] == len(t["cid"]) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
            assert all(lo % cc.KCTILE for lo, _ in runs[1:])  # the cuts lie inside tiles
    assert cc.count_share(1, 0, 2) == (0, 0) and cc.count_share(1, 1, 2) == (0, 1)  # a rank without an entry
    # by identity: pairs that share a head, counters on either side of ci and of cs
    for rc in (big, cases["count lists of 4096 and 4100"]):
        follows = np.flatnonzero(rc.head != np.arange(len(rc.head)))
        assert len(follows) > 200 and np.array_equal(rc.head[follows], follows - 1) and np.all(rc.kmer_lo[follows] == rc.kmer_lo[follows - 1])
        assert not rc.kmer_hi.any() and np.all(rc.kmer_lo >> np.uint64(40) == 0) and np.all(rc.kmer_lo & np.uint64(3) == 0)  # A ... A
        for ci in (1, 2, 3):
            for cs in (0, 3):
                counts = cc.counters(rc, ci, cs)
                assert set(counts.tolist()) == {0, ci - 1, ci, cs, cs + 1, 0xFFFFFFFF}
                m = cc.matched_by_identity(counts, rc.head, ci, cs)
                assert 0 < m.sum() < len(m) and (counts[follows] != counts[follows - 1]).sum() > 100
                assert np.array_equal(m[follows], m[follows - 1])
