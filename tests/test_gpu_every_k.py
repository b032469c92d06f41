"""-m gpu: every per-k instantiation of the hot-path kernels against the oracle, one test id per k.  The kernels are templates on k
(k_count_kmers<K>: mg_kcount.hip, dispatch_kc; k_sketch_reads<K, HM>: mg_sketch_kernel.h, dispatch_k and mg_sketch_cmash.hip;
k_hash_positions<K, HM>: the genome side), and what changes with K — the flank of a candidate (kc_flank: steps at k = 19, 23, 53 and
every second k above), the candidates per window, the LDS stage of k + 15 bases per lane, the k - 1 overlap of a long read's chunks,
the registers — is where one K can go wrong while its neighbours hold.  The k ranges come from the library: the sweep covers
[KMER_MATCH_MIN_K, KMER_MATCH_MAX_K] (identity) and [1, MAX_K] (sketch), and test_the_k_ranges_are_the_librarys holds the native
refusals to exactly those bounds, so a wider range fails here until the sweep covers it.  Bit-exact: integer work throughout."""
import re

import numpy as np
import pytest

import util
from metalign_amd import _hip
from metalign_amd.distributed import KMER_MATCH_DEFAULT_FROM_K, KMER_MATCH_MAX_K, KMER_MATCH_MIN_K
from test_gpu_kcount import _add_tiles, _check_counts

pytestmark = pytest.mark.gpu

K_IDENTITY = list(range(KMER_MATCH_MIN_K, KMER_MATCH_MAX_K + 1))
K_SKETCH = list(range(1, _hip.MAX_K + 1))
K_MODE1 = _hip.hash_mode1_ks()  # hash mode 1 and the forward-selected sketches are built for these k only
U64_MAX = _hip.U64_MAX
NTILES, LAST = 40, 37


@pytest.fixture(scope="module")
def count_case(oracle_lib):
    """get(k) -> the identity sample of k (built once; the oracle's counts cached per cs): genomes with homopolymers and tandem repeats
    (and, at even k, a reverse-palindromic k-mer planted in genome 2 and filed in its table entries); a table of ks = [max(4, k - 10), k],
    selected by the forward hash where the library builds one; 40 tiles of every kind (the last of 37 reads) laid out so that one
    workgroup's wavefronts walk every pair of util.TILE_TRANSITIONS, one of them the edge reads of k."""
    cache = {}

    def get(k):
        if k in cache:
            return cache[k]
        rng = np.random.default_rng(9700 + k)
        gb, go = util.tile_genomes(rng)
        pal = util.palindrome(rng, k) if k % 2 == 0 else None
        if pal is not None:
            at = int(go[2]) + 7000
            gb[at:at + k] = np.frombuffer(pal, dtype=np.uint8)
        sketch_hash = "forward" if k in K_MODE1 else "canonical"
        entries = oracle_lib.sketch_genomes_kmers(gb, go, k, 300, sketch_hash=sketch_hash)
        if pal is not None:
            entries = util.with_entry(entries, 2, pal, int(oracle_lib.kmer_hashes(pal, k)[0][0]))
        ks = [max(4, k - 10), k]
        want_table = oracle_lib.refpipe_build(*entries, ks)
        h, khi, klo, o = entries
        pick = rng.choice(np.arange(int(o[0]), int(o[6])), size=6, replace=False)
        kmers = [util.unpack_kmer(khi[i], klo[i], k) for i in pick]
        kinds = util.tile_kinds_walked(rng, NTILES)
        kinds[NTILES - 2] = "edge"
        rb, ro = util.edge_sample(rng, gb, go, kinds, k, util.edge_reads(rng, gb, go, k, kmers, pal), last=LAST)
        c = cache[k] = dict(kinds=kinds, rb=rb, ro=ro, entries=entries, ks=ks, want_table=want_table, pal=pal, sketch_hash=sketch_hash, want={})
        for cs in (3, 0):
            c["want"][cs] = oracle_lib.refpipe_count_kmers(rb, ro, k, want_table["kmer_hi"], want_table["kmer_lo"], cs=cs)
        return c
    return get


@pytest.mark.parametrize("k", K_IDENTITY)
def test_count_kmers_at_every_k(hip, oracle_lib, knobs, count_case, k):
    """k_count_kmers<k>: per-pair counts, the k-mers seen and every column equal the oracle's at cs 3 and 0, on kc_grid 1 (ten tiles to a
    wavefront) and the launcher's grid, in one add and in three tile-aligned adds into one set of counters; the hash path on the same
    reads gives the same columns."""
    c = count_case(k)
    assert set(c["kinds"]) == set(util.TILE_KINDS) | {"edge"} and len(c["ro"]) - 1 == (NTILES - 1) * util.TILE + LAST
    missing = util.TILE_TRANSITIONS - util.tile_transitions(c["kinds"], 1)
    assert not missing, missing
    table = hip.refdb_build(*c["entries"], c["ks"])
    table.index_kmers()
    assert table.has_kmer_index and 0 < table.distinct_kmers <= len(c["entries"][0])
    if c["pal"] is not None:  # the palindrome is a pair of the table, and the reads hold it
        hi, lo = util.pack_kmer(c["pal"])
        at = np.flatnonzero((c["want_table"]["kmer_hi"] == np.uint64(hi)) & (c["want_table"]["kmer_lo"] == np.uint64(lo)))
        assert len(at) and c["want"][3][0][at].min() == 3
    try:
        for cs in (3, 0):
            want, seen = c["want"][cs]
            assert want.max() == 3 if cs == 3 else want.max() > 3
            assert (want == 0).sum() > 0 and (want > 0).sum() > 0
            hip.count_saturation(cs)
            for grid in (1, 0):
                knobs("kc_grid", grid)
                for pieces in (1, 3):
                    kc = table.kmer_counts()
                    _add_tiles(hip, kc, c["rb"], c["ro"], pieces)
                    _check_counts(hip, oracle_lib, kc, table, want, seen, c["want_table"], cs,
                                  "k=%d %s cs=%d kc_grid=%d adds=%d" % (k, c["sketch_hash"], cs, grid, pieces))
                    kc.free()
        hip.count_saturation(3)
        knobs("kc_grid", 0)
        d_b, d_o = hip.array(np.concatenate([c["rb"], np.zeros(64, np.uint8)])), hip.array(c["ro"])
        sk = hip.sketch_reads_dev(d_b.ptr, d_o.ptr, len(c["ro"]) - 1, k, table.max_hash, 0)
        hits_h, sizes_h = hip.refpipe_containment(sk, table, 2)
        kc = table.kmer_counts()
        _add_tiles(hip, kc, c["rb"], c["ro"], 1)
        hits_k, sizes_k = hip.refpipe_containment_counts(kc, table, 2)
        assert np.array_equal(hits_h, hits_k) and np.array_equal(sizes_h, sizes_k), k
        assert hits_k[-1].sum() > 0
        for x in (sk, kc, d_b, d_o):
            x.free()
    finally:
        hip.count_saturation(3)
        table.free()


# ---- the read sketch: k_sketch_reads<K, HM> through its three walks of a tile (tests/test_gpu_edges.py: test_sketch_three_walks_of_a_tile)
@pytest.fixture(scope="module")
def walk_case():
    """get(k) -> [(name, bases, offsets)]: 960 equal reads of 150 bases, the same count ragged (empty reads, reads of k - 1), the equal
    ones with a few N (some tiles with an invalid base, most without).  Built once per k for both hash modes."""
    cache = {}

    def get(k):
        if k not in cache:
            rng = np.random.default_rng(9800 + k)
            gb, go = util.random_genomes(rng, 5, 6000)
            uniform = util.sample_reads(rng, gb, go, 960, 150, err=0.01)[:2]
            rb, ro, _ = util.sample_reads(rng, gb, go, 960, 150, err=0.01, ragged=True, lower=True)
            lens = np.diff(ro).astype(np.int64)
            lens[::37] = 0
            lens[5::41] = k - 1
            keep = np.concatenate([np.arange(int(ro[i]), int(ro[i]) + lens[i]) for i in range(len(lens))])
            ragged = (rb[keep], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
            dirty = uniform[0].copy()
            dirty[rng.integers(0, dirty.size, size=8)] = ord("N")
            cache[k] = [("uniform",) + uniform, ("ragged",) + ragged, ("dirty", dirty, uniform[1])]
        return cache[k]
    return get


def _walks_equal_the_oracle(hip, oracle_lib, knobs, cases, k, top):
    """Every walk, at a fractional hmax and at hmax = max (once cut to the 300 smallest), on the launcher's path and the forced list
    path: hashes, counts, truncation and k-mers seen."""
    for force_list in (0, 1):
        knobs("force_list", force_list)
        for name, b, o in cases:
            d_b, d_o = hip.array(b if b.size else np.zeros(1, np.uint8)), hip.array(o)
            for hmax, s in ((int(0.05 * top), 0), (U64_MAX, 0), (U64_MAX, 300)):
                oh, oc, otr, oseen = oracle_lib.sketch_reads(b, o, k, hmax=hmax, s=s)
                sk = hip.sketch_reads_dev(d_b.ptr, d_o.ptr, len(o) - 1, k, hmax, s)
                gh, gc = sk.download()
                case = (k, name, hex(hmax), s, "list" if force_list else "launcher's path")
                assert np.array_equal(gh, oh) and np.array_equal(gc, oc), case
                assert (sk.truncated, sk.kmers_seen) == (otr, oseen), case
                assert len(oh) > 0 or hmax != U64_MAX, case
                sk.free()
            d_b.free()
            d_o.free()
    knobs("force_list", 0)


@pytest.mark.parametrize("k", K_SKETCH)
def test_sketch_reads_at_every_k(hip, oracle_lib, knobs, walk_case, k):
    _walks_equal_the_oracle(hip, oracle_lib, knobs, walk_case(k), k, 2.0**64)


@pytest.fixture
def mode1(hip, oracle_lib):
    """Hash mode 1 in the library and the oracle; mode 0 again afterwards, whatever happened."""
    try:
        hip.set_hash_mode(1)
        oracle_lib.set_hash_mode(1)
        yield
    finally:
        hip.set_hash_mode(0)
        oracle_lib.set_hash_mode(0)


@pytest.mark.parametrize("k", K_MODE1)
def test_sketch_reads_under_hash_mode_1_at_every_listed_k(hip, oracle_lib, knobs, walk_case, mode1, k):
    _walks_equal_the_oracle(hip, oracle_lib, knobs, walk_case(k), k, oracle_lib.CMASH_PRIME)


# ---- the genome side: k_hash_positions<K, HM> (plain, forward-selected, CMash)
def _genomes(k):
    """Genomes of 3000, 0, k - 1, k, 2000 (with N runs and lower case) and 500 bases.  -> (bases, offsets)"""
    rng = np.random.default_rng(9900 + k)
    lens = [3000, 0, k - 1, k, 2000, 500]
    parts = [rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).astype(np.uint8) for n in lens]
    parts[4][100:110] = ord("N")
    parts[4][700:701] = ord("N")
    parts[4][1200:1300] |= 0x20
    return np.concatenate(parts), np.cumsum([0] + lens).astype(np.uint64)


def _genome_side_equals_the_oracle(hip, oracle_lib, k, n, variants):
    gb, go = _genomes(k)
    h, o = hip.sketch_genomes(gb, go, k, n)
    oh, oo = oracle_lib.sketch_genomes(gb, go, k, n)
    assert np.array_equal(o, oo) and np.array_equal(h, oh), k
    assert o[2] == o[1] and o[3] == o[2] and o[4] - o[3] == 1, k  # no window in 0 or k - 1 bases; one in k
    for sketch_hash in variants:
        got = hip.sketch_genomes_kmers(gb, go, k, n, sketch_hash=sketch_hash)
        want = oracle_lib.sketch_genomes_kmers(gb, go, k, n, sketch_hash=sketch_hash)
        for a, b, what in zip(got, want, ("hashes", "kmer_hi", "kmer_lo", "offsets")):
            assert np.array_equal(a, b), (k, sketch_hash, what)


@pytest.mark.parametrize("k", K_SKETCH)
def test_genome_sketch_at_every_k(hip, oracle_lib, k):
    _genome_side_equals_the_oracle(hip, oracle_lib, k, 200, ("canonical",) if k >= 4 else ())


@pytest.mark.parametrize("k", K_MODE1)
def test_forward_selected_genome_sketch_at_every_listed_k(hip, oracle_lib, k):
    _genome_side_equals_the_oracle(hip, oracle_lib, k, 200, ("forward",))


@pytest.mark.parametrize("k", K_MODE1)
def test_genome_sketch_under_hash_mode_1_at_every_listed_k(hip, oracle_lib, mode1, k):
    _genome_side_equals_the_oracle(hip, oracle_lib, k, 200, ("canonical", "forward"))


# ---- the bounds
def _refused(fn, *args):
    """-> the (lo, hi) the error names: fn must raise a HipError of MG_ERR_ARG whose message holds '[lo, hi]'."""
    with pytest.raises(_hip.HipError) as e:
        fn(*args)
    assert e.value.code == _hip.ERR_ARG, str(e.value)
    m = re.search(r"\[(\d+), ?(\d+)\]", str(e.value))
    assert m, str(e.value)
    return int(m.group(1)), int(m.group(2))


def test_the_k_ranges_are_the_librarys(hip, oracle_lib):
    """The index refuses a table of k_max just outside [KMER_MATCH_MIN_K, KMER_MATCH_MAX_K] and names that range; the read sketch and the
    genome sketch refuse k just outside [1, MAX_K] and name it; the tables refuse a k above MAX_K.  After every refusal the next valid
    call gives the oracle's answer — at the bounds themselves."""
    rng = np.random.default_rng(9950)
    gb, go = util.random_genomes(rng, 4, 3000)
    rb, ro, _ = util.sample_reads(rng, gb, go, 300, 150, err=0.01, present=[1, 2])
    lo, hi = K_IDENTITY[0], K_IDENTITY[-1]

    def counts_equal_the_oracle(k):
        entries = oracle_lib.sketch_genomes_kmers(gb, go, k, 100)
        want_table = oracle_lib.refpipe_build(*entries, [k])
        want, seen = oracle_lib.refpipe_count_kmers(rb, ro, k, want_table["kmer_hi"], want_table["kmer_lo"])
        table = hip.refdb_build(*entries, [k])
        table.index_kmers()
        kc = table.kmer_counts()
        _add_tiles(hip, kc, rb, ro, 1)
        assert np.array_equal(kc.download(), want) and kc.stats()["kmers"] == seen and want.sum() > 0, k
        kc.free()
        table.free()

    below = oracle_lib.sketch_genomes_kmers(gb, go, lo - 1, 100)
    t = hip.refdb_build(*below, [lo - 1])
    assert _refused(t.index_kmers) == (lo, hi)
    assert not t.has_kmer_index
    t.free()
    counts_equal_the_oracle(lo)
    entries = oracle_lib.sketch_genomes_kmers(gb, go, hi, 100)
    assert _refused(hip.refdb_build, *entries, [hi + 1]) == (1, _hip.MAX_K)
    built = hip.refdb_build(*entries, [hi])
    got = built.download()
    up = hip.refdb_upload([hi + 1], 4, got["pair_hash"], got["pair_gen"], got["gsize"], built.max_hash, [])  # (a stored table says its k)
    assert _refused(up.index_kmers, got["kmer_hi"], got["kmer_lo"]) == (lo, hi)
    up.free()
    built.free()
    counts_equal_the_oracle(hi)

    for k in (0, _hip.MAX_K + 1):
        assert _refused(hip.sketch_reads, rb, ro, k) == (K_SKETCH[0], K_SKETCH[-1])
        assert _refused(hip.sketch_genomes, gb, go, k, 100) == (K_SKETCH[0], K_SKETCH[-1])
        for kk in (K_SKETCH[0], K_SKETCH[-1]):
            assert all(np.array_equal(a, b) for a, b in zip(hip.sketch_reads(rb, ro, kk), oracle_lib.sketch_reads(rb, ro, kk))), kk
            assert all(np.array_equal(a, b) for a, b in zip(hip.sketch_genomes(gb, go, kk, 100), oracle_lib.sketch_genomes(gb, go, kk, 100))), kk


@pytest.mark.parametrize("kmax", [KMER_MATCH_DEFAULT_FROM_K - 1, KMER_MATCH_DEFAULT_FROM_K])
def test_select_main_on_either_side_of_the_default_switch(hip, tmp_path, monkeypatch, kmax):
    """select_main on a reference-pipeline table of k_max just below and at KMER_MATCH_DEFAULT_FROM_K: the default (the hash path below,
    by identity from there on), `--kmer_match hash` and `--kmer_match identity_only` write the same CSV."""
    from metalign_amd import build_db, select_db
    from test_gpu_bam_reads import _select_csv
    from test_pipeline_gpu import _make_data_dir
    rng = np.random.default_rng(9960 + kmax)
    data, gb, go, names, accs = _make_data_dir(tmp_path, rng)
    rb, ro, _ = util.sample_reads(rng, gb, go, 3000, 150, err=0.005, present=[3, 8])
    fq = tmp_path / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(rb[int(ro[i]):int(ro[i + 1])]), b"I" * int(ro[i + 1] - ro[i]))
                            for i in range(len(ro) - 1)))
    tdir = str(data / "sketch_table_ref")
    build_db.main([str(data / "organism_files"), tdir, "-n", "150", "-k", "%d,%d" % (kmax - 10, kmax), "--reference_pipeline"])
    chose = []
    applies = select_db.kmer_match_applies
    monkeypatch.setattr(select_db, "kmer_match_applies", lambda *a: chose.append(applies(*a)) or chose[-1])
    csvs = [_select_csv(select_db, fq, data, tdir, tmp_path / ("t%d" % i), extra)
            for i, extra in enumerate(([], ["--kmer_match", "hash"], ["--kmer_match", "identity_only"]))]
    assert chose == [kmax >= KMER_MATCH_DEFAULT_FROM_K, False, True]
    assert csvs[0].count(b"\n") > 2
    assert csvs[1] == csvs[0] and csvs[2] == csvs[0]
