"""GPU parity of stage A BY K-MER IDENTITY (mg_kcount.hip: the minimizer-partitioned count of the reads' k_max-mers against the
table's k-mers, what `kmc` + `kmc_tools intersect` compute, scripts/select_db.py:50-59) against the oracle's
mgo_refpipe_count_kmers, through the C ABI: per-pair counts, KMC's total of k-mers, the columns of every k, and the hash path
(mg_sketch_* + mg_refpipe_containment_dev) on the same inputs.  Bit-exact: integer work throughout."""
import re

import numpy as np
import pytest

from util import TILE, TILE_TRANSITIONS, flat, random_genomes, refpipe_case, sample_reads, tile_genomes, tile_kinds, tile_sample, tile_transitions

pytestmark = pytest.mark.gpu

K_SETS = [[21, 31, 51], [30, 40, 50, 60], [15], [16, 17], [5, 33, 64], [32], [20, 47], [31, 32, 33, 63]]


def _counts(hip, table, reads, pieces=1):
    kc = table.kmer_counts()
    step = (len(reads) + pieces - 1) // pieces
    keep = []
    for a in range(0, max(len(reads), 1), max(step, 1)):
        rb, ro = flat(reads[a:a + step])
        d_b, d_o = hip.array(np.concatenate([rb, np.zeros(64, np.uint8)])), hip.array(ro)
        kc.add_dev(d_b.ptr, d_o.ptr, len(ro) - 1, int(ro[-1]))
        keep += [d_b, d_o]
    hip.sync()
    for x in keep:
        x.free()
    return kc


# (tables selected by the forward hash are built for a list of k: include/metalign_hip.h, mg_sketch_genomes_kmers_forward)
CASES = [(ks, "canonical") for ks in K_SETS] + [(ks, "forward") for ks in ([21, 31, 51], [30, 40, 50, 60], [15], [5, 33, 64], [32])]


@pytest.mark.parametrize("ks,sketch_hash", CASES, ids=str)
def test_counts_and_columns_match_the_oracle(hip, oracle_lib, ks, sketch_hash):
    rng = np.random.default_rng(6100 + 17 * sum(ks) + len(sketch_hash))
    genomes, reads = refpipe_case(rng)
    kmax, n = ks[-1], 150
    gb, go = flat(genomes)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, kmax, n, sketch_hash=sketch_hash)
    table = hip.refdb_build(h, khi, klo, o, ks)
    want_table = oracle_lib.refpipe_build(h, khi, klo, o, ks)
    table.index_kmers()
    assert table.has_kmer_index and 0 < table.distinct_kmers <= len(h)
    rb, ro = flat(reads)
    for cs in (3, 0, 1):
        hip.count_saturation(cs)
        try:
            want, seen = oracle_lib.refpipe_count_kmers(rb, ro, kmax, want_table["kmer_hi"], want_table["kmer_lo"], cs=cs)
            kc = _counts(hip, table, reads, pieces=3 if cs == 3 else 1)
            got = kc.download()
            st = kc.stats()
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
            assert st["kmers"] == seen
            assert want.max() >= (cs if cs else 2)
            for ci in (1, 2, 3):
                if cs and ci > cs:
                    continue
                hits, sizes = hip.refpipe_containment_counts(kc, table, ci)
                whits, wsizes = oracle_lib.refpipe_containment_counts(want, ci, want_table)
                assert np.array_equal(hits, whits), (ks, cs, ci)
                assert np.array_equal(sizes, wsizes)
            kc.free()
        finally:
            hip.count_saturation(3)
    # the hash path on the same inputs: the same columns (no two k-mers of this table share a hash)
    d_b, d_o = hip.array(np.concatenate([rb, np.zeros(64, np.uint8)])), hip.array(ro)
    sk = hip.sketch_reads_dev(d_b.ptr, d_o.ptr, len(reads), kmax, table.max_hash, 0)
    hits_h, sizes_h = hip.refpipe_containment(sk, table, 2)
    kc = _counts(hip, table, reads)
    hits_k, sizes_k = hip.refpipe_containment_counts(kc, table, 2)
    assert np.array_equal(hits_h, hits_k) and np.array_equal(sizes_h, sizes_k)
    # heads: a pair counts at the first pair with its k-mer
    heads = table.kmer_heads()
    assert np.all(heads <= np.arange(len(heads))) and np.array_equal(heads[heads], heads)
    for x in (sk, kc, table, d_b, d_o):
        x.free()


def test_an_uploaded_table_is_indexed_from_its_stored_kmers(hip, oracle_lib):
    ks = [21, 31, 51]
    rng = np.random.default_rng(6200)
    genomes, reads = refpipe_case(rng)
    gb, go = flat(genomes)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], 150)
    built = hip.refdb_build(h, khi, klo, o, ks)
    got = built.download()
    up = hip.refdb_upload(ks, len(genomes), got["pair_hash"], got["pair_gen"], got["gsize"], built.max_hash, [got["small"][k] for k in ks[:-1]])
    with pytest.raises(Exception):
        up.index_kmers()  # an uploaded table does not hold its k-mers
    up.index_kmers(got["kmer_hi"], got["kmer_lo"])
    built.index_kmers()
    a, b = _counts(hip, up, reads), _counts(hip, built, reads)
    assert np.array_equal(a.download(), b.download())
    ha, _ = hip.refpipe_containment_counts(a, up, 2)
    hb, _ = hip.refpipe_containment_counts(b, built, 2)
    assert np.array_equal(ha, hb) and ha.sum() > 0
    for x in (a, b, up, built):
        x.free()


@pytest.mark.parametrize("kind", ["long", "tiny_stage", "one_read", "none", "all_n"])
def test_reads_of_every_shape(hip, oracle_lib, kind):
    """Reads longer than 1023 (taken through in chunks), a batch whose average length sizes a stage the longest read does not
    fit, a single read, no read at all, reads of N only."""
    ks, n = [31, 51], 200
    rng = np.random.default_rng(6300 + len(kind))
    gb, go = random_genomes(rng, 6, 6000)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], n)
    table = hip.refdb_build(h, khi, klo, o, ks)
    want_table = oracle_lib.refpipe_build(h, khi, klo, o, ks)
    table.index_kmers()
    g = [bytes(gb[int(go[i]):int(go[i + 1])]) for i in range(6)]
    if kind == "long":
        reads = [g[0][:2500], g[1][100:1400], g[2][:1023], g[2][:1024], g[3], g[0][:2500]] + [g[4][i:i + 150] for i in range(0, 3000, 50)]
    elif kind == "tiny_stage":
        reads = [g[0][i:i + 60] for i in range(0, 5000, 7)] + [g[1][:900]] + [g[0][i:i + 60] for i in range(0, 5000, 7)]
    elif kind == "one_read":
        reads = [g[5][200:350]]
    elif kind == "none":
        reads = []
    else:
        reads = [b"N" * 150] * 70 + [g[0][:150], g[0][:150]]
    rb, ro = flat(reads)
    want, seen = oracle_lib.refpipe_count_kmers(rb, ro, ks[-1], want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    kc = _counts(hip, table, reads) if reads else table.kmer_counts()
    got = kc.download()
    assert np.array_equal(got, want)
    assert kc.stats()["kmers"] == seen
    if kind in ("long", "tiny_stage"):
        assert want.sum() > 0
    kc.reset()
    hip.sync()
    assert kc.download().sum() == 0 and kc.stats()["kmers"] == 0
    kc.free()
    table.free()


def test_a_larger_sample_against_a_larger_table(hip, oracle_lib):
    """40 genomes x 500 sketched k-mers, 30 000 reads of 150 bp with errors from a few of them, both strands: every pair's count."""
    ks = [30, 40, 50, 60]
    rng = np.random.default_rng(6400)
    gb, go = random_genomes(rng, 40, 20000)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], 500)
    table = hip.refdb_build(h, khi, klo, o, ks)
    want_table = oracle_lib.refpipe_build(h, khi, klo, o, ks)
    table.index_kmers()
    rb, ro, _ = sample_reads(rng, gb, go, 30000, 150, err=0.01, present=[1, 5, 7, 30])
    reads = [bytes(rb[int(ro[i]):int(ro[i + 1])]) for i in range(len(ro) - 1)]
    want, seen = oracle_lib.refpipe_count_kmers(rb, ro, ks[-1], want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    kc = _counts(hip, table, reads, pieces=2)
    assert np.array_equal(kc.download(), want)
    st = kc.stats()
    assert st["kmers"] == seen and st["matches"] > 0
    hits, sizes = hip.refpipe_containment_counts(kc, table, 2)
    whits, wsizes = oracle_lib.refpipe_containment_counts(want, 2, want_table)
    assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes)
    assert set(np.argsort(-hits[-1].astype(np.int64))[:4]) == {1, 5, 7, 30}
    kc.free()
    table.free()


def test_three_hundred_samples_through_one_set_of_counters(hip, oracle_lib):
    """The entry counters are not zeroed between samples: their words carry a pass number of eight bits (mg_kcount_core.h:
    kc_entry_count) and are zeroed when it wraps.  300 resets of one set of counters, two samples in turn — one that saturates its
    k-mers, one that barely touches them: every sample's counts are its own, before, at and after the wrap."""
    ks = [31, 51]
    rng = np.random.default_rng(6500)
    gb, go = random_genomes(rng, 8, 8000)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], 300)
    table = hip.refdb_build(h, khi, klo, o, ks)
    want_table = oracle_lib.refpipe_build(h, khi, klo, o, ks)
    table.index_kmers()
    samples = []
    for present, n in (([1, 4], 6000), ([6], 300)):
        rb, ro, _ = sample_reads(rng, gb, go, n, 150, err=0.01, present=present)
        want, _ = oracle_lib.refpipe_count_kmers(rb, ro, ks[-1], want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
        samples.append((hip.array(np.concatenate([rb, np.zeros(64, np.uint8)])), hip.array(ro), len(ro) - 1, int(ro[-1]), want))
    assert samples[0][4].max() == 3 and 0 < samples[1][4].sum() < samples[0][4].sum()
    kc = table.kmer_counts()
    for i in range(300):
        d_b, d_o, n, nb, want = samples[i & 1]
        kc.reset()
        kc.add_dev(d_b.ptr, d_o.ptr, n, nb)
        if i < 4 or i % 37 == 0 or 250 <= i <= 262 or i >= 296:
            assert np.array_equal(kc.download(), want), i
    kc.free()
    table.free()


# ---- many tiles per wavefront: k_count_kmers is persistent (a wavefront walks tile after tile, carrying its LDS stage, not-a-base
# bits, run lists and totals from one to the next), and at its own grid every test above gives a wavefront one tile at most.
# kc_grid (a test hook) cuts the grid to 1, 2 or 5 workgroups: 78, 39 or 16 tiles to a wavefront, of every kind util.tile_sample makes.
TILE_KSETS = {15: [15], 31: [21, 31], 32: [16, 32], 33: [21, 33], 51: [21, 31, 51], 64: [30, 40, 64]}
TILE_CASES = [(k, cs) for k in TILE_KSETS for cs in (3, 0)] + [(31, 1)]


@pytest.fixture(scope="module")
def tiled(oracle_lib):
    """get(k_max, cs) -> the tile-by-tile sample of that k_max (313 tiles, the last of 37 reads), its table's entries and the
    oracle's (counts, k-mers seen) at cs: built once for the module, shared by every grid."""
    cache = {}

    def get(kmax, cs):
        if kmax not in cache:
            rng = np.random.default_rng(6600 + kmax)
            gb, go = tile_genomes(rng)
            kinds = tile_kinds(rng, 313)
            rb, ro = tile_sample(rng, gb, go, kinds, kmax, last=37)
            entries = oracle_lib.sketch_genomes_kmers(gb, go, kmax, 1500)
            cache[kmax] = dict(kinds=kinds, rb=rb, ro=ro, entries=entries, want_table=oracle_lib.refpipe_build(*entries, TILE_KSETS[kmax]),
                               want={})
        c = cache[kmax]
        if cs not in c["want"]:
            c["want"][cs] = oracle_lib.refpipe_count_kmers(c["rb"], c["ro"], kmax, c["want_table"]["kmer_hi"], c["want_table"]["kmer_lo"], cs=cs)
        return c
    return get


def _add_tiles(hip, kc, rb, ro, pieces):
    """The reads into one set of counters in `pieces` adds, split at tile boundaries (the last add takes the partial tile)."""
    n = len(ro) - 1
    cut = [min(n, (n // TILE) * i // pieces * TILE) for i in range(pieces)] + [n]
    keep = []
    for a, b in zip(cut, cut[1:]):
        o = (ro[a:b + 1] - ro[a]).astype(np.uint64)
        d_b, d_o = hip.array(np.concatenate([rb[int(ro[a]):int(ro[b])], np.zeros(64, np.uint8)])), hip.array(o)
        kc.add_dev(d_b.ptr, d_o.ptr, b - a, int(o[-1]))
        keep += [d_b, d_o]
    hip.sync()
    for x in keep:
        x.free()


def _check_counts(hip, oracle_lib, kc, table, want, seen, want_table, cs, case):
    got = kc.download()
    assert np.array_equal(got, want), (case, np.flatnonzero(got != want)[:10])
    assert kc.stats()["kmers"] == seen, case
    for ci in (1, 2, 3):
        if cs and ci > cs:
            continue
        hits, sizes = hip.refpipe_containment_counts(kc, table, ci)
        whits, wsizes = oracle_lib.refpipe_containment_counts(want, ci, want_table)
        assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes), (case, ci)


@pytest.mark.parametrize("kmax,cs", TILE_CASES)
def test_counts_tile_by_tile_with_many_tiles_per_wavefront(hip, oracle_lib, tiled, knobs, kmax, cs):
    """Tiles of every kind in turn through each wavefront (kc_grid 1, 2, 5 and the launcher's own grid), the sample counted in one add
    and in three into one set of counters: per-pair counts, the k-mers seen and every column equal the oracle's."""
    c = tiled(kmax, cs)
    want, seen = c["want"][cs]
    assert want.max() > 3 if cs == 0 else want.max() == cs
    assert (want == 0).sum() > 0
    for grid in (1, 2, 5):
        missing = TILE_TRANSITIONS - tile_transitions(c["kinds"], grid)
        assert not missing, (grid, missing)
    table = hip.refdb_build(*c["entries"], TILE_KSETS[kmax])
    table.index_kmers()
    hip.count_saturation(cs)
    try:
        for grid in (1, 2, 5, 0):
            knobs("kc_grid", grid)
            for pieces in (1, 3):
                kc = table.kmer_counts()
                _add_tiles(hip, kc, c["rb"], c["ro"], pieces)
                _check_counts(hip, oracle_lib, kc, table, want, seen, c["want_table"], cs,
                              "k=%d cs=%d kc_grid=%d adds=%d" % (kmax, cs, grid, pieces))
                kc.free()
    finally:
        hip.count_saturation(3)
        table.free()


def _short_reads(rng, gb, go, n, present):
    """n reads of 60-100 bp from the genomes `present`, both strands, 1 % substitutions (vectorised: half a million of them)."""
    lens = rng.integers(60, 101, size=n)
    src = np.asarray(present)[rng.integers(0, len(present), size=n)]
    glen = (go[1:] - go[:-1]).astype(np.int64)
    start = go[src].astype(np.int64) + (rng.random(n) * (glen[src] - 100)).astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(gb, 100)[start].copy()
    rev = rng.random(n) < 0.5
    comp = np.zeros(256, np.uint8)
    comp[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"TGCA", np.uint8)
    win[rev] = comp[win[rev, ::-1]]
    err = rng.random(win.shape) < 0.01
    win[err] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(err.sum()))
    rb = win[np.arange(100)[None, :] < lens[:, None]]
    ro = np.zeros(n + 1, dtype=np.uint64)
    ro[1:] = np.cumsum(lens)
    return rb, ro


def test_counts_at_the_launchers_grid_with_several_tiles_per_wavefront(hip, oracle_lib, tiled):
    """Enough short reads (60-100 bp, k = 31) that the launcher's own grid — at most three workgroups of four wavefronts per CU — gives every
    wavefront two tiles or more; and the same reads on a stage-A stream at one workgroup per CU (how distributed.py runs stage A):
    every pair's count and the k-mers seen equal the oracle's.  And the tile-by-tile sample under that production cap."""
    ncu = int(re.search(r"(\d+) CUs", hip.device_name()).group(1))
    ntiles = int(np.ceil(2.5 * 4 * 3 * ncu)) + 1
    nreads = (ntiles - 1) * TILE + 17
    assert (nreads + TILE - 1) // TILE >= 2.5 * 4 * 3 * ncu
    rng = np.random.default_rng(6700)
    gb, go = tile_genomes(rng)
    rb, ro = _short_reads(rng, gb, go, nreads, present=[0, 2, 5, 7])
    entries = oracle_lib.sketch_genomes_kmers(gb, go, 31, 1500)
    want_table = oracle_lib.refpipe_build(*entries, [21, 31])
    want, seen = oracle_lib.refpipe_count_kmers(rb, ro, 31, want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    assert want.max() == 3
    table = hip.refdb_build(*entries, [21, 31])
    table.index_kmers()
    c = tiled(31, 3)
    try:
        kc = table.kmer_counts()
        _add_tiles(hip, kc, rb, ro, 1)
        _check_counts(hip, oracle_lib, kc, table, want, seen, want_table, 3, "launcher's grid, %d tiles, %d CUs" % (ntiles, ncu))
        kc.free()
        hip.stage_a_side_stream(3)
        hip.stage_a_workgroups_per_cu(1)
        kc = table.kmer_counts()
        _add_tiles(hip, kc, rb, ro, 1)
        _check_counts(hip, oracle_lib, kc, table, want, seen, want_table, 3, "stage-A stream, one workgroup per CU")
        kc.free()
        t2 = hip.refdb_build(*c["entries"], TILE_KSETS[31])
        t2.index_kmers()
        for pieces in (1, 3):
            kc = t2.kmer_counts()
            _add_tiles(hip, kc, c["rb"], c["ro"], pieces)
            _check_counts(hip, oracle_lib, kc, t2, *c["want"][3], c["want_table"], 3, "tiles, stage-A stream, one workgroup per CU, adds=%d" % pieces)
            kc.free()
        t2.free()
    finally:
        hip.stage_a_side_stream(0)
        hip.stage_a_workgroups_per_cu(0)
        table.free()


def test_stage_b_with_many_tiles_per_workgroup(hip, oracle_lib, knobs):
    """k_contain_pairs (hash path: the largest k's column and the marks of the smaller k), k_match_pairs (by identity) and
    k_refpipe_count (the smaller k's columns) walk 2 048 pairs to a tile: a table of 40 genomes x 500 k-mers per k, 4 k, on kb_grid
    1 and 3 workgroups (10 tiles and more to each) and the launcher's grid equals the oracle at ci 1, 2 and 3."""
    ks = [30, 40, 50, 60]
    rng = np.random.default_rng(6800)
    gb, go = random_genomes(rng, 40, 20000)
    entries = oracle_lib.sketch_genomes_kmers(gb, go, ks[-1], 500)
    h, _, _, o = entries
    want_table = oracle_lib.refpipe_build(*entries, ks)
    assert len(want_table["pair_hash"]) >= 8 * 2048 and all(len(want_table["small"][k]["cid"]) >= 2 * 2048 for k in ks[:-1])
    kinds = tile_kinds(rng, 160)
    rb, ro = tile_sample(rng, gb, go, kinds, ks[-1], last=50, main=3, present=(3, 9, 17, 22, 35))
    oh, oc, otr, _ = oracle_lib.sketch_reads(rb, ro, ks[-1], hmax=int(h.max()))
    want, _ = oracle_lib.refpipe_count_kmers(rb, ro, ks[-1], want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    table = hip.refdb_build(*entries, ks)
    table.index_kmers()
    db = hip.upload_table(h, o)
    d_b, d_o = hip.array(np.concatenate([rb, np.zeros(64, np.uint8)])), hip.array(ro)
    sk = hip.sketch_reads_dev(d_b.ptr, d_o.ptr, len(ro) - 1, ks[-1], table.max_hash, 0)
    kc = table.kmer_counts()
    _add_tiles(hip, kc, rb, ro, 1)
    assert np.array_equal(kc.download(), want)
    for grid in (1, 3, 0):
        knobs("kb_grid", grid)
        for ci in (1, 2, 3):
            case = "kb_grid=%d ci=%d" % (grid, ci)
            hits, sizes = hip.refpipe_containment(sk, table, ci)
            whits, wsizes = oracle_lib.refpipe_containment(oh, oc, ci, want_table)
            assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes), ("hash path", case)
            assert all(w.sum() > 0 for w in whits), case
            hits, sizes = hip.refpipe_containment_counts(kc, table, ci)
            whits, wsizes = oracle_lib.refpipe_containment_counts(want, ci, want_table)
            assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes), ("by identity", case)
            hits, sizes = hip.containment(sk, db, ci)
            whits, wsizes = oracle_lib.containment(oh, oc, otr, ci, h, o)
            assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes), ("one k", case)
    for x in (sk, kc, db, table, d_b, d_o):
        x.free()
