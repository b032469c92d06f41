"""-m gpu: stage B (mg_contain.hip) held to its definition at every tile, run and bucket edge (tests/contain_cases.py; what each
family reaches is shown by test_contain_cases_host.py).  Every case goes through the library at ci = 1, 2, 3, at the launcher's
grid and with one workgroup walking every tile (kb_grid = 1), on a fresh sketch handle (the call builds the bucket index) and again
on the same handle (cached index), through both table uploads, alone and beside other cases in one containment_multi_dev call.
Equality with the definition is exact everywhere; outputs lie in front of a guard word.

The reference pipeline's cases run on the hash path and by k-mer identity with hand-made counters, whole and in set_count_share
runs, and the count step alone over hand-made prefix bitmaps.  (By identity the table without a pair is left out: an index over no
k-mer is stage A's business.)"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import contain_cases as cc

pytestmark = pytest.mark.gpu

SENT32 = 0xA5A5A5A5
CIS = (1, 2, 3)
CASES = [(fam, c.name) for fam, make in cc.FAMILIES.items() for c in make()]


@functools.lru_cache(maxsize=None)
def _want(family, name, ci):
    """The definition over a case: computed once, shared by every test that needs it."""
    return cc.want(cc.case(family, name), ci)


def _sketch(hip, c, k=21):
    """A fresh handle made the way the case says; it holds what the case says the library makes of the feed."""
    n = len(c.feed_hashes)
    d_h = hip.array(c.feed_hashes if n else np.zeros(1, np.uint64))
    d_c = hip.array(c.feed_counts if n else np.zeros(1, np.uint32))
    try:
        sk = hip.sketch_from_pairs_dev(d_h.ptr, d_c.ptr, n, k, s=c.s)
    finally:
        d_h.free()
        d_c.free()
    if getattr(c, "set_bound", None) is not None:
        sk.set_bound(*c.set_bound)
    return sk


def _tables(hip, c, both=True):
    max_hash = int(c.pair_hash[-1]) if len(c.pair_hash) else 0
    out = {"hash-major": hip.upload_table_sorted(c.pair_hash, c.pair_gen, c.gsize, max_hash)}
    if both:
        out["genome-major"] = hip.upload_table(*cc.genome_major(c))  # (k_pair_genomes, k_genome_sizes)
    return out


def _contain(hip, sketches, tables, ci):
    """One call over all of them -> [(hits, sizes)], the guards behind the outputs checked."""
    outs = [(hip.array(np.full(t.ngenomes + 1, SENT32, np.uint32)), hip.array(np.full(t.ngenomes + 1, SENT32, np.uint32))) for t in tables]
    try:
        if len(tables) == 1:
            hip.containment_dev(sketches[0], tables[0], ci, outs[0][0].ptr, outs[0][1].ptr)
        else:
            hip.containment_multi_dev(sketches, tables, ci, [o[0].ptr for o in outs], [o[1].ptr for o in outs])
        hip.sync()
        got = []
        for t, (d_h, d_s) in zip(tables, outs):
            h, s = d_h.download(), d_s.download()
            assert h[t.ngenomes] == SENT32 and s[t.ngenomes] == SENT32
            got.append((h[:t.ngenomes], s[:t.ngenomes]))
        return got
    finally:
        for d_h, d_s in outs:
            d_h.free()
            d_s.free()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), ("hits",) + what + (np.flatnonzero(got[0] != want[0])[:8].tolist(),)
    assert np.array_equal(got[1], want[1]), ("sizes",) + what + (np.flatnonzero(got[1] != want[1])[:8].tolist(),)


@pytest.mark.parametrize("family,name", CASES)
def test_every_case_alone(hip, knobs, family, name):
    c = cc.case(family, name)
    tables = _tables(hip, c)
    try:
        sk = _sketch(hip, c)  # the handle is what the case says it is
        h, n = sk.download()
        assert sk.size == len(c.q_hashes) and np.array_equal(h, c.q_hashes) and np.array_equal(n, c.q_counts)
        assert sk.truncated == c.truncated and sk.last_hash == (int(c.q_hashes[-1]) if len(c.q_hashes) else 0)
        sk.free()
        for grid in (0, 1):
            knobs("kb_grid", grid)  # 0: the launcher's grid; 1: one workgroup walks every tile
            for upload, table in tables.items():
                for ci in CIS:
                    sk = _sketch(hip, c)
                    try:
                        for index in ("built by this call", "cached"):
                            _same(_contain(hip, [sk], [table], ci)[0], _want(family, name, ci), (name, upload, ci, grid, index))
                    finally:
                        sk.free()
    finally:
        for t in tables.values():
            t.free()


@pytest.mark.parametrize("group", list(cc.MULTI))
def test_cases_beside_each_other_in_one_call(hip, knobs, group):
    members = cc.MULTI[group]
    cases = [cc.case(f, n) for f, n in members]
    tables = [_tables(hip, c, both=False)["hash-major"] for c in cases]
    try:
        for grid in (0, 1):
            knobs("kb_grid", grid)
            for ci in CIS:
                sketches = [_sketch(hip, c) for c in cases]
                try:
                    for index in ("built by this call", "cached"):
                        got = _contain(hip, sketches, tables, ci)
                        for (f, n), g in zip(members, got):
                            _same(g, _want(f, n, ci), (group, n, ci, grid, index))
                    # ... and each of them alone on the handle whose index the multi call built
                    for (f, n), sk, t in zip(members, sketches, tables):
                        _same(_contain(hip, [sk], [t], ci)[0], _want(f, n, ci), (group, n, ci, grid, "alone after"))
                finally:
                    for sk in sketches:
                        sk.free()
    finally:
        for t in tables:
            t.free()


# ---------------------------------------------------------------- the reference pipeline's table
RNAMES = [rc.name for rc in cc.refpipe()]
RefSketch = namedtuple("RefSketch", "feed_hashes feed_counts s")


def _refcase(name):
    return {rc.name: rc for rc in cc.refpipe()}[name]


def _reftable(hip, rc):
    max_hash = int(rc.pair_hash[-1]) if len(rc.pair_hash) else 0
    return hip.refdb_upload(rc.ks, rc.ngenomes, rc.pair_hash, rc.pair_gen, rc.gsize, max_hash, rc.small)


class _Columns:
    """nk pairs of output buffers with a guard word behind ngenomes."""

    def __init__(self, hip, nk, g):
        self.g = g
        self.h = [hip.array(np.full(g + 1, SENT32, np.uint32)) for _ in range(nk)]
        self.s = [hip.array(np.full(g + 1, SENT32, np.uint32)) for _ in range(nk)]

    def got(self, rows=None):
        hits, sizes = [], []
        for d_h, d_s in list(zip(self.h, self.s))[:rows]:
            h, s = d_h.download(), d_s.download()
            assert h[self.g] == SENT32 and s[self.g] == SENT32
            hits.append(h[:self.g])
            sizes.append(s[:self.g])
        return np.array(hits, dtype=np.uint32).reshape(len(hits), self.g), np.array(sizes, dtype=np.uint32).reshape(len(sizes), self.g)

    def free(self):
        for d in self.h + self.s:
            d.free()


def _by_hash(hip, sk, table, rc, ci):
    out = _Columns(hip, len(rc.ks), rc.ngenomes)
    try:
        hip.refpipe_containment_dev(sk, table, ci, [d.ptr for d in out.h], [d.ptr for d in out.s])
        hip.sync()
        return out.got()
    finally:
        out.free()


@pytest.mark.parametrize("name", RNAMES)
def test_refpipe_cases_on_the_hash_path(hip, knobs, name):
    rc = _refcase(name)
    table = _reftable(hip, rc)
    feed = RefSketch(rc.q_hashes, rc.q_counts, 0)
    try:
        for grid in (0, 1):
            knobs("kb_grid", grid)
            for ci in CIS:
                matched = cc.matched_by_hash(rc.q_hashes, rc.q_counts, ci, rc.pair_hash)
                want = cc.refpipe_expected(rc, matched)
                sk = _sketch(hip, feed, rc.ks[-1])
                try:
                    for index in ("built by this call", "cached"):
                        _same(_by_hash(hip, sk, table, rc, ci), want, (name, ci, grid, index))
                    if grid:
                        continue
                    # runs of the count lists that begin and end inside tiles: each rank's part, and the parts add up
                    for world in cc.REFPIPE_WORLDS:
                        total = np.zeros_like(want[0])
                        for rank in range(world):
                            table.set_count_share(rank, world)
                            got = _by_hash(hip, sk, table, rc, ci)
                            part = cc.refpipe_expected(rc, matched, rank, world)
                            _same(got, part, (name, ci, "rank %d of %d" % (rank, world)))
                            total += got[0]
                        assert np.array_equal(total[:-1], want[0][:-1]) and np.array_equal(total[-1], world * want[0][-1])
                    table.set_count_share(0, 1)
                finally:
                    table.set_count_share(0, 1)
                    sk.free()
    finally:
        table.free()


@pytest.mark.parametrize("name", [n for n in RNAMES if n != "no pairs"])
def test_refpipe_cases_by_identity_with_hand_made_counters(hip, knobs, name):
    rc = _refcase(name)
    table = _reftable(hip, rc)
    m = len(rc.small)
    try:
        table.index_kmers(rc.kmer_hi, rc.kmer_lo)
        assert np.array_equal(table.kmer_heads(), rc.head)  # a k-mer is counted at the first pair that holds it
        for cs in (0, 3):
            hip.count_saturation(cs)
            for grid in (0, 1):
                knobs("kb_grid", grid)
                for ci in CIS:
                    counts = cc.counters(rc, ci, cs)
                    want = cc.refpipe_expected(rc, cc.matched_by_identity(counts, rc.head, ci, cs))
                    d_c = hip.array(counts)
                    out = _Columns(hip, m + 1, rc.ngenomes)
                    try:
                        hip.refpipe_mark_counts_dev(d_c.ptr, table, ci, out.h[m].ptr, out.s[m].ptr)
                        hip.refpipe_count_dev(table, None, [d.ptr for d in out.h[:m]], [d.ptr for d in out.s[:m]])
                        hip.sync()
                        _same(out.got(), want, (name, ci, cs, grid))
                    finally:
                        out.free()
                        d_c.free()
    finally:
        hip.count_saturation(3)
        table.free()


@pytest.mark.parametrize("name", RNAMES)
def test_the_count_step_over_hand_made_bitmaps(hip, knobs, name):
    """One bit either side of a word of the bitmap, the last bit, every bit but one, all and none."""
    rc = _refcase(name)
    if not rc.small:
        return
    table = _reftable(hip, rc)
    m = len(rc.small)
    try:
        patterns = [("none", lambda npre: np.zeros(npre, bool)), ("all", lambda npre: np.ones(npre, bool))]
        for p in (0, 31, 32, 63, -1):
            patterns.append(("only %d" % p, lambda npre, p=p: np.arange(npre) == (p % npre if p < 0 else p)))
            patterns.append(("all but %d" % p, lambda npre, p=p: np.arange(npre) != (p % npre if p < 0 else p)))
        for grid in (0, 1):
            knobs("kb_grid", grid)
            for what, make in patterns:
                marked = [make(t["nprefix"]) for t in rc.small]
                d_m = [hip.array(np.concatenate([cc.mark_words(mk), np.zeros(1, np.uint32)])) for mk in marked]
                out = _Columns(hip, m, rc.ngenomes)
                try:
                    for again in (0, 1):  # (the second count follows no mark call: it zeroes its counters itself)
                        hip.refpipe_count_dev(table, [d.ptr for d in d_m], [d.ptr for d in out.h], [d.ptr for d in out.s])
                        hip.sync()
                        hits, sizes = out.got()
                        for s, t in enumerate(rc.small):
                            assert np.array_equal(hits[s], cc.count_hits(marked[s], t, rc.ngenomes)), (name, what, grid, s, again)
                            assert np.array_equal(sizes[s], t["gsize"]), (name, what, grid, s, again)
                finally:
                    out.free()
                    for d in d_m:
                        d.free()
    finally:
        table.free()
