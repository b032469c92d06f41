"""-m gpu: the device-side calls that exist only for a multi-GPU job, ONE BY ONE and in-process against numpy / the oracle —
the calls tests/dist_two_ranks_one_gpu.py and tests/dist_config3_full.py reach only through ShardJob, from child processes, at one
set of shapes:
  * mg_kcounts_pack2_dev / _merge2_dev / _pack2_bytes (k_kc_pack2, k_kc_merge2): the ragged last dword (npairs % 16 != 0), fewer than
    16 pairs, counters above 3, up to 33 ranks, a stride longer than the array; the natural exchange of W read shares;
  * mg_sketch_slice_words_dev (k_slice_words): 0 to 4096 bounds on resolved, pending, truncated, merged, empty and hand-made sketches,
    bounds on present hashes, repeated, at and above 2^63; the overflow word of a pending sketch;
  * mg_sketch_set_bound through stage B (k_upper_bound_one, the count_sizes path of containment_launch);
  * mg_containment_multi_dev: tables of unequal size, with no genome, with no pair; sketches empty, pending, truncated;
  * mg_refdb_set_count_share: worlds up to beyond the shortest count list;
  * mg_profile_map_words_dev and mg_filter_use_resident.
Integer work throughout: every comparison is np.array_equal."""
import ctypes

import numpy as np
import pytest

import shard_ref
from metalign_amd import _hip, synth
from metalign_amd.distributed import table_bounds, table_max_hash, table_slice
from util import flat, random_genomes, refpipe_case, sample_reads

pytestmark = pytest.mark.gpu

U64_MAX = 0xFFFFFFFFFFFFFFFF
SENT32 = 0xA5A5A5A5
SENT64 = 0x5A5A5A5A5A5A5A5A


def _h2d(hip, d_ptr, host):
    host = np.ascontiguousarray(host)
    hip._chk(hip.lib.mg_memcpy_h2d(ctypes.c_void_p(int(d_ptr)), ctypes.c_void_p(host.ctypes.data), ctypes.c_uint64(host.nbytes)))


def _d2h(hip, d_ptr, count, dtype):
    out = np.empty(count, dtype=dtype)
    hip._chk(hip.lib.mg_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(int(d_ptr)), ctypes.c_uint64(out.nbytes)))
    return out


@pytest.fixture()
def held():
    """held(x, ...) -> x, ...: device buffers and handles of one test, freed when the test ends, however it ends."""
    mine = []

    def hold(*xs):
        mine.extend(xs)
        return xs[0] if len(xs) == 1 else xs
    yield hold
    for x in reversed(mine):
        x.free()


def _reads_dev(hip, rb, ro):
    """(bases, offsets) on the device, the bases padded as the counting kernel's callers pad them."""
    return hip.array(np.concatenate([np.asarray(rb, np.uint8), np.zeros(64, np.uint8)])), hip.array(ro)


# ---------------------------------------------------------------- 1. two-bit counter exchange
def _pack_table(hip, shape, ks=(31, 51), n=150):
    """A reference-pipeline table with its k-mer index whose number of pairs is ragged / below 16 / a multiple of 16; some
    k-mers in more than one genome, so that some pair's head is another pair."""
    rng = np.random.default_rng(7100 + len(shape))
    if shape == "tiny":
        seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=ks[-1] + 8).tobytes()]
    else:
        gb, go = random_genomes(rng, 6, 3000)
        seqs = [bytes(gb[int(go[i]):int(go[i + 1])]) for i in range(6)]
        seqs.append(seqs[0][:1500] + seqs[1][1500:])   # shares k-mers with two others
        if shape == "even":
            seqs.append(seqs[2][::-1])
    gb, go = flat(seqs)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], n)
    table = hip.refdb_build(h, khi, klo, o, list(ks))
    table.index_kmers()
    return table


def _pack2_numpy(raw):
    """min(c, 3) of pair i in bits 2 (i & 15) of dword i >> 4; the unused bits of the last dword zero."""
    n = len(raw)
    f = np.zeros((n + 15) // 16 * 16, dtype=np.uint32)
    f[:n] = np.minimum(raw, 3)
    return (f.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def _fields(words, n):
    return ((words[:, None] >> (2 * np.arange(16, dtype=np.uint32))) & np.uint32(3)).reshape(-1)[:n]


@pytest.mark.parametrize("shape", ["ragged", "tiny", "even"])
def test_pack2_and_merge2_on_written_counters(hip, held, shape):
    table = held(_pack_table(hip, shape))
    npairs = table.sizes()[0]
    assert {"ragged": npairs % 16 != 0 and npairs > 16, "tiny": 0 < npairs < 16, "even": npairs % 16 == 0 and npairs > 0}[shape], npairs
    heads = table.kmer_heads()
    if shape != "tiny":
        assert np.any(heads != np.arange(npairs))
    nd = (npairs + 15) // 16
    rng = np.random.default_rng(7200 + npairs)
    kc = held(table.kmer_counts())
    try:
        ptr, cnt = kc.device()
        assert cnt == npairs
        hd = np.unique(heads)
        raw = np.zeros(npairs, dtype=np.uint32)
        raw[hd] = rng.choice(np.array([0, 1, 2, 3, 4, 7, 2 ** 32 - 1], dtype=np.uint32), size=len(hd))
        raw[hd[0]], raw[heads[npairs - 1]] = 2 ** 32 - 1, 7
        assert np.any(raw > 3)
        kc.wait()
        hip.sync()
        _h2d(hip, ptr, raw)
        # ---- pack
        assert kc.pack2_bytes() == 4 * nd
        d_out = held(hip.array(np.full(nd + 1, SENT32, dtype=np.uint32)))
        kc.pack2_dev(d_out.ptr)
        hip.sync()
        got = d_out.download()
        assert got[nd] == SENT32
        assert np.array_equal(got[:nd], _pack2_numpy(raw))
        if npairs % 16:
            assert int(got[nd - 1]) >> (2 * (npairs % 16)) == 0
        assert np.array_equal(_d2h(hip, ptr, npairs, np.uint32), raw)  # (the counters themselves are left alone)
        # ---- merge: the ranks' arrays random in every bit (the unused ones of the last dword too), sentinel padding between them
        for nranks in (1, 2, 5, 8, 33):
            for stride in (nd, nd + 3):
                every = np.full(nranks * stride, 0xFFFFFFFF, dtype=np.uint32)
                words = rng.integers(0, 2 ** 32, size=(nranks, nd), dtype=np.uint64).astype(np.uint32)
                every.reshape(nranks, stride)[:, :nd] = words
                want = np.zeros(npairs, dtype=np.uint32)
                for r in range(nranks):
                    want += _fields(words[r], npairs)
                d_all = held(hip.array(every))
                _h2d(hip, ptr, np.full(npairs + 1, SENT32, dtype=np.uint32))  # (the counters have one word behind the pairs')
                kc.merge2_dev(d_all.ptr, nranks, 4 * stride)
                kc.wait()
                hip.sync()
                after = _d2h(hip, ptr, npairs + 1, np.uint32)
                assert after[npairs] == SENT32, (nranks, stride)
                assert np.array_equal(after[:npairs], want), (nranks, stride)
                for cs in (1, 2, 3):
                    hip.count_saturation(cs)
                    try:
                        assert np.array_equal(kc.download(), np.minimum(want[heads], cs)), (nranks, stride, cs)
                    finally:
                        hip.count_saturation(3)
        # ---- refusals
        d_all = held(hip.array(np.zeros(2 * nd, dtype=np.uint32)))
        try:
            for cs in (0, 7):
                hip.count_saturation(cs)
                with pytest.raises(_hip.HipError):
                    kc.pack2_dev(d_out.ptr)
        finally:
            hip.count_saturation(3)
        with pytest.raises(_hip.HipError):
            kc.merge2_dev(d_all.ptr, 2, 4 * (nd - 1))
        with pytest.raises(_hip.HipError):
            kc.merge2_dev(d_all.ptr, 0, 4 * nd)
        _h2d(hip, ptr, np.zeros(npairs + 1, dtype=np.uint32))
    finally:
        hip.count_saturation(3)


@pytest.fixture(scope="module")
def count_case(hip, oracle_lib):
    """One reference-pipeline table (k = 21, 31, 51) with its k-mer index, the oracle's, one read set and its counts."""
    rng = np.random.default_rng(7300)
    genomes, reads = refpipe_case(rng)
    ks = [21, 31, 51]
    gb, go = flat(genomes)
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], 40)
    table = hip.refdb_build(h, khi, klo, o, ks)
    table.index_kmers()
    want_table = oracle_lib.refpipe_build(h, khi, klo, o, ks)
    rb, ro = flat(reads)
    want, _ = oracle_lib.refpipe_count_kmers(rb, ro, ks[-1], want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    columns = oracle_lib.refpipe_containment_counts(want, 2, want_table)
    try:
        yield dict(table=table, want_table=want_table, reads=reads, want=want, columns=columns, ks=ks)
    finally:
        table.free()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_pack2_merge2_of_read_shares(hip, oracle_lib, count_case, held, world):
    """What ShardJob._sum_kmer_counts does at cs = 3, without the collective: every rank counts its share of the reads, packs, the
    arrays lie one behind the other, every rank merges.  min(sum of min(c_r, 3), 3) = min(sum c_r, 3)."""
    table, want_table, reads, want = (count_case[x] for x in ("table", "want_table", "reads", "want"))
    kmax = count_case["ks"][-1]
    npairs = table.sizes()[0]
    nd = (npairs + 15) // 16
    cuts = [len(reads) * r // world for r in range(world + 1)]
    d_all = held(hip.array(np.full(world * nd + 1, SENT32, dtype=np.uint32)))
    occurs_in = np.zeros(npairs, dtype=np.int64)
    for r in range(world):
        rb, ro = flat(reads[cuts[r]:cuts[r + 1]])
        occurs_in += oracle_lib.refpipe_count_kmers(rb, ro, kmax, want_table["kmer_hi"], want_table["kmer_lo"], cs=0)[0] > 0
        d_b, d_o = held(*_reads_dev(hip, rb, ro))
        kc = held(table.kmer_counts())
        kc.add_dev(d_b.ptr, d_o.ptr, len(ro) - 1, int(ro[-1]))
        assert kc.pack2_bytes() == 4 * nd
        kc.pack2_dev(d_all.ptr + 4 * r * nd)
    assert occurs_in.max() > 1  # some k-mer is counted by more than one rank: the sum does something
    merged = held(table.kmer_counts())
    merged.merge2_dev(d_all.ptr, world, 4 * nd)
    assert np.array_equal(merged.download(), want)
    assert d_all.download()[world * nd] == SENT32
    hits, sizes = hip.refpipe_containment_counts(merged, table, 2)
    whits, wsizes = count_case["columns"]
    assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes) and whits[-1].max() > 0
    # the raw pointer, as a job hands over counters it summed itself
    g = table.ngenomes
    d_h, d_s = held(hip.array(np.full(g + 1, SENT32, np.uint32)), hip.array(np.full(g + 1, SENT32, np.uint32)))
    ptr, cnt = merged.device()
    merged.wait()
    hip.refpipe_mark_counts_dev(ptr, table, 2, d_h.ptr, d_s.ptr)
    hip.sync()
    gh, gs = d_h.download(), d_s.download()
    assert cnt == npairs and gh[g] == SENT32 and gs[g] == SENT32
    assert np.array_equal(gh[:g], whits[-1]) and np.array_equal(gs[:g], wsizes[-1])


# ---------------------------------------------------------------- 2. slice words
NBOUNDS = (0, 1, 7, 255, 256, 257, 1000, 4096)


def _bounds(rng, h, nb):
    """nb ascending bounds: first of all one ON a present hash, twice; then below the first hash, above the last, around 2^63, the
    ends of the range; then present hashes (some twice: runs of repeated bounds) and random values."""
    first = [2 ** 63, 2 ** 64 - 1, 0, 2 ** 63 - 1, 2 ** 63 + 1]
    if len(h):
        mid = int(h[len(h) // 2])
        first = [mid, mid, max(int(h[0]), 1) - 1, min(int(h[-1]), U64_MAX - 1) + 1] + first + [int(h[0]), int(h[-1])]
    present = rng.choice(h, size=nb // 3) if len(h) else np.zeros(0, np.uint64)
    cand = np.concatenate([np.array(first, dtype=np.uint64), present, present[: len(present) // 2],
                           rng.integers(0, 2 ** 64, size=nb + 1, dtype=np.uint64)])
    return np.sort(cand[:nb])


def _want_words(h, truncated, b):
    """-> (the nbounds + 5 words as uint64, the cut positions)"""
    cuts = np.searchsorted(h, b, side="left").astype(np.uint64)
    edges = np.concatenate([np.zeros(1, np.uint64), cuts, np.array([len(h)], np.uint64)])
    tail = np.array([int(truncated), int(h[-1]) if len(h) else 0, len(h), 0], dtype=np.uint64)
    return np.concatenate([np.diff(edges), tail]), cuts


def _slice_words_all(hip, sk, d_bounds):
    """slice_words_dev for every set of bounds, queued one behind the other: nothing reads anything back until all are queued."""
    outs = []
    try:
        for d_b, nb in d_bounds:
            outs.append(hip.array(np.full(nb + 6, SENT64, dtype=np.uint64)))
            sk.slice_words_dev(d_b.ptr, nb, outs[-1].ptr)
        hip.sync()
        return [d_w.download() for d_w in outs]
    finally:
        for d_w in outs:
            d_w.free()


def _reads_go_pending(hip, knobs, d_b, d_o, nreads, k, hmax, s, hint):
    """Whether sketch_reads_dev_async hands these inputs back PENDING.  The C ABI has no query for that and every accessor resolves,
    so a pending handle that resolves cleanly looks like one that never was pending; what only a pending handle can do is report a
    rebuild.  The same call on the same inputs, its counting table sized for one candidate in a million (the sketch's buffers then
    hold 1024 entries, the caller asserts more distinct hashes than that), must report one: the planner sends these inputs through
    the counting table, and every asynchronous call that goes through the table comes back pending.  hint: the knob's value afterwards."""
    knobs("distinct_hint_ppm", 1)
    twin = hip.sketch_reads_dev_async(d_b.ptr, d_o.ptr, nreads, k, hmax, s)
    knobs("distinct_hint_ppm", hint)
    try:
        return twin.resolve()
    finally:
        twin.free()


def _merge_goes_pending(hip, ph, k, lo, hi, outside):
    """The same for sketch_merge_dev_async over [lo, hi]: as many pairs and the same declared range (all its planner looks at), one
    pair moved to `outside`, far from the range.  The counting table loses that pair and the handle, resolved, reports a rebuild."""
    assert not lo <= outside <= hi
    twin_h = ph.copy()
    twin_h[0] = outside
    d_h, d_c = hip.array(twin_h), hip.array(np.ones(len(ph), np.uint32))
    twin = hip.sketch_merge_dev_async(d_h.ptr, d_c.ptr, len(ph), k, lo, hi)
    try:
        return twin.resolve()
    finally:
        for x in (twin, d_h, d_c):
            x.free()


def _check_slice_words(hip, held, sk, h, truncated, pending, seed):
    """h / truncated: what the sketch must hold.  pending: the handle has not been resolved by anybody yet (the caller has shown, with
    _reads_go_pending / _merge_goes_pending, that its inputs give a pending one): the words are asked for before and after resolve()."""
    rng = np.random.default_rng(seed)
    sets = [_bounds(rng, h, nb) for nb in NBOUNDS]
    if len(h):
        assert all(np.isin(b, h).any() for b in sets if len(b))                      # a bound equal to a present hash
        assert all((b[1:] == b[:-1]).any() for b in sets if len(b) >= 7)              # repeated bounds
        assert all((b[0] < h[0] or h[0] == 0) and b[-1] > h[-1] for b in sets if len(b) >= 7)  # below the first hash, above the last
    assert all((b >= 2 ** 63).any() for b in sets if len(b) >= 7)
    d_bounds = [(held(hip.array(b if len(b) else np.zeros(1, np.uint64))), len(b)) for b in sets]
    rounds = [_slice_words_all(hip, sk, d_bounds)] if pending else []
    if pending:
        assert not sk.resolve()
    rounds.append(_slice_words_all(hip, sk, d_bounds))
    assert sk.size == len(h) and sk.truncated == bool(truncated)
    for got in rounds:
        for b, w in zip(sets, got):
            want, cuts = _want_words(h, truncated, b)
            assert w[len(b) + 5] == SENT64, len(b)
            assert np.array_equal(w[: len(b) + 5], want), (len(b), np.flatnonzero(w[: len(b) + 5] != want)[:8])
            assert sk.split([int(x) for x in b]) == [int(x) for x in cuts], len(b)
    d_big, d_w = held(hip.array(np.zeros(4097, np.uint64)), hip.empty(4097 + 5, np.uint64))
    with pytest.raises(_hip.HipError):
        sk.slice_words_dev(d_big.ptr, 4097, d_w.ptr)


@pytest.fixture(scope="module")
def slice_reads(hip, oracle_lib):
    """Reads of one short genome at high coverage: enough windows that the deferred sketch goes through the counting table (it stays
    pending), a few thousand distinct k-mers, hashes over the whole 64-bit range."""
    rng = np.random.default_rng(7400)
    gb, go = random_genomes(rng, 1, 4000)
    rb, ro, _ = sample_reads(rng, gb, go, 500, 150, err=0.0)
    assert rb.size >= 2 * 32768  # (the table path, hence a pending handle, from 32768 expected candidates on)
    assert len(oracle_lib.sketch_reads(rb, ro, 21)[0]) > 2048  # (more distinct hashes than a starved table's sketch holds)
    d_b, d_o = hip.array(rb), hip.array(ro)
    try:
        yield dict(rb=rb, ro=ro, d_b=d_b, d_o=d_o, nreads=len(ro) - 1)
    finally:
        d_b.free()
        d_o.free()


@pytest.mark.parametrize("s", [0, 500])
@pytest.mark.parametrize("how", ["resolved", "pending"])
def test_slice_words_of_a_read_sketch(hip, oracle_lib, slice_reads, knobs, held, how, s):
    c, k = slice_reads, 21
    knobs("distinct_hint_ppm", 1000000)  # (the counting table sized for every candidate, whatever earlier sketches of this k held)
    if how == "pending":
        assert _reads_go_pending(hip, knobs, c["d_b"], c["d_o"], c["nreads"], k, U64_MAX, s, 1000000)
    h, _, truncated, _ = oracle_lib.sketch_reads(c["rb"], c["ro"], k, s=s)
    assert 2000 < len(h) < 10000 if s == 0 else (len(h) == s and truncated)
    assert h[0] < 2 ** 63 <= h[-1] or s
    fn = hip.sketch_reads_dev if how == "resolved" else hip.sketch_reads_dev_async
    sk = held(fn(c["d_b"].ptr, c["d_o"].ptr, c["nreads"], k, U64_MAX, s))
    _check_slice_words(hip, held, sk, h, truncated, how == "pending", 7410 + s)
    gh, _ = sk.download()
    assert np.array_equal(gh, h)


def test_slice_words_of_a_pending_merge(hip, held):
    """mg_sketch_merge_dev_async over a declared range that straddles 2^63 (the table path: pending from 32768 pairs on)."""
    rng = np.random.default_rng(7420)
    lo, hi = 2 ** 62, 2 ** 63 + 2 ** 62
    a = np.unique(rng.integers(lo, hi, size=30000, dtype=np.uint64))
    b = np.unique(np.concatenate([rng.choice(a, size=5000, replace=False), rng.integers(lo, hi, size=15000, dtype=np.uint64)]))
    ph = np.concatenate([a, b])
    assert len(ph) >= 32768
    h = np.unique(ph)
    assert len(h) < len(ph) and h[0] < 2 ** 63 <= h[-1]
    assert _merge_goes_pending(hip, ph, 21, lo, hi - 1, 0)
    d_h, d_c = held(hip.array(ph), hip.array(np.ones(len(ph), np.uint32)))
    sk = held(hip.sketch_merge_dev_async(d_h.ptr, d_c.ptr, len(ph), 21, lo, hi - 1))
    _check_slice_words(hip, held, sk, h, False, True, 7421)
    gh, gc = sk.download()
    assert np.array_equal(gh, h) and np.array_equal(gc, np.where(np.isin(h, a) & np.isin(h, b), 2, 1))


def test_slice_words_of_an_empty_and_a_chosen_sketch(hip, held):
    d_b, d_o = held(hip.array(np.zeros(1, np.uint8)), hip.array(np.zeros(1, np.uint64)))
    for fn in (hip.sketch_reads_dev, hip.sketch_reads_dev_async):
        sk = held(fn(d_b.ptr, d_o.ptr, 0, 21, U64_MAX, 0))
        _check_slice_words(hip, held, sk, np.zeros(0, np.uint64), False, False, 7430)
    h = np.array([0, 1, 5, 2 ** 62, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 3, 2 ** 64 - 2], dtype=np.uint64)
    perm = np.random.default_rng(7431).permutation(len(h))
    d_h, d_c = held(hip.array(h[perm]), hip.array(np.ones(len(h), np.uint32)))
    sk = held(hip.sketch_from_pairs_dev(d_h.ptr, d_c.ptr, len(h), 21))
    _check_slice_words(hip, held, sk, h, False, False, 7432)
    # every bound on or next to an entry
    b = np.sort(np.concatenate([h, h, h[1:] - np.uint64(1), h + np.uint64(1)]))
    d_bounds = held(hip.array(b))
    got = _slice_words_all(hip, sk, [(d_bounds, len(b))])[0]
    assert np.array_equal(got[: len(b) + 5], _want_words(h, False, b)[0])


def test_slice_words_report_a_table_overflow(hip, oracle_lib, knobs, held):
    """A counting table sized far too small (knob distinct_hint_ppm): the words published before resolve() carry the overflow count,
    resolve() reports the rebuild, and the words asked for again are the oracle's."""
    rng = np.random.default_rng(7440)
    gb, go = random_genomes(rng, 1, 30000)
    rb, ro, _ = sample_reads(rng, gb, go, 800, 150, err=0.01)
    k = 21
    h, _, truncated, _ = oracle_lib.sketch_reads(rb, ro, k)
    assert len(h) > 30000
    d_b, d_o = held(hip.array(rb), hip.array(ro))
    b = _bounds(rng, h, 7)
    d_bounds = held(hip.array(b))
    knobs("distinct_hint_ppm", 500)
    sk = held(hip.sketch_reads_dev_async(d_b.ptr, d_o.ptr, len(ro) - 1, k, U64_MAX, 0))
    knobs("distinct_hint_ppm", 0)
    before = _slice_words_all(hip, sk, [(d_bounds, len(b))])[0]
    assert before[len(b) + 4] != 0 and before[len(b) + 5] == SENT64
    assert sk.resolve()
    after = _slice_words_all(hip, sk, [(d_bounds, len(b))])[0]
    assert np.array_equal(after[: len(b) + 5], _want_words(h, truncated, b)[0])


# ---------------------------------------------------------------- 3. completeness bound through stage B
@pytest.fixture(scope="module")
def bound_case(hip, oracle_lib):
    """40 genomes x 100 hashes at k = 21 and a read sketch under the table's largest hash with more than 32768 entries (sequencing
    errors make them), so that its merge over the whole range is a pending one."""
    rng = np.random.default_rng(7500)
    k, n, G = 21, 100, 40
    gb, go = random_genomes(rng, G, 400)
    dbh, dbo = oracle_lib.sketch_genomes(gb, go, k, n)
    hmax = table_max_hash(dbh, dbo)
    rb, ro, _ = sample_reads(rng, gb, go, 4000, 150, err=0.03, present=np.arange(0, G, 2))
    qh, qc, _, _ = oracle_lib.sketch_reads(rb, ro, k, hmax=hmax)
    assert len(qh) > 32768 and qc.max() == 3 and qc.min() == 1
    return dict(k=k, G=G, dbh=dbh, dbo=dbo, hmax=hmax, qh=qh, qc=qc, rb=rb, ro=ro)


def _bounded(sh, so, qh, qc, truncated, bound, ci):
    """oracle.containment's rules with the bound given from outside: sizes[g] = #{h of g's slice: h <= B}, hits[g] = those that are
    in the read sketch's slice with count >= ci.  Not truncated: no bound."""
    G = len(so) - 1
    gen = np.repeat(np.arange(G), np.diff(so.astype(np.int64)))
    keep = sh <= np.uint64(bound) if truncated else np.ones(len(sh), bool)
    if len(qh):
        pos = np.minimum(np.searchsorted(qh, sh), len(qh) - 1)
        present = (qh[pos] == sh) & (qc[pos] >= ci)
    else:
        present = np.zeros(len(sh), bool)
    return (np.bincount(gen[keep & present], minlength=G).astype(np.uint32), np.bincount(gen[keep], minlength=G).astype(np.uint32))


def _run_bounded(hip, sk, table, G, truncated, bound, ci=2):
    sk.set_bound(truncated, bound)
    d_h, d_s = hip.array(np.full(G + 1, SENT32, np.uint32)), hip.array(np.full(G + 1, SENT32, np.uint32))
    try:
        hip.containment_dev(sk, table, ci, d_h.ptr, d_s.ptr)
        hip.sync()
        gh, gs = d_h.download(), d_s.download()
    finally:
        d_h.free()
        d_s.free()
    assert gh[G] == SENT32 and gs[G] == SENT32
    return gh[:G], gs[:G]


def test_set_bound_on_a_slice(hip, oracle_lib, bound_case, held):
    c = bound_case
    G, dbh, dbo, qh, qc = c["G"], c["dbh"], c["dbo"], c["qh"], c["qc"]
    srt = np.sort(dbh)
    lo, hi = int(srt[len(srt) // 4]), int(srt[3 * len(srt) // 4])
    sh, so = table_slice(dbh, dbo, lo, hi)
    inq = (qh >= np.uint64(lo)) & (qh < np.uint64(hi))
    sqh, sqc = qh[inq], qc[inq]
    table = held(hip.upload_table(sh, so))
    d_h, d_c = held(hip.array(sqh), hip.array(sqc))
    sk = held(hip.sketch_from_pairs_dev(d_h.ptr, d_c.ptr, len(sqh), c["k"]))
    ssh = np.sort(sh)
    on_hash = int(ssh[len(ssh) // 2])
    matched = ssh[np.isin(ssh, sqh[sqc >= 2])]
    on_matched = int(matched[len(matched) // 2])
    assert on_hash in sh and on_matched in sqh and lo > 0 and int(ssh[0]) >= lo
    seen = set()
    for truncated, bound in [(1, on_hash), (1, on_hash - 1), (1, on_matched), (1, on_matched - 1), (1, int(ssh[0])), (1, int(ssh[-1])),
                             (1, int(ssh[0]) - 1), (1, 0), (1, U64_MAX), (1, U64_MAX - 1), (0, int(ssh[len(ssh) // 8])), (0, 0)]:
        hits, sizes = _run_bounded(hip, sk, table, G, truncated, bound)
        whits, wsizes = _bounded(sh, so, sqh, sqc, truncated, bound, 2)
        assert np.array_equal(sizes, wsizes), (truncated, bound)
        assert np.array_equal(hits, whits), (truncated, bound)
        seen.add((int(wsizes.sum()), int(whits.sum())))
    # the bound moved sizes and hits: on a hash against one below it, none against all
    a, b = _bounded(sh, so, sqh, sqc, 1, on_matched, 2), _bounded(sh, so, sqh, sqc, 1, on_matched - 1, 2)
    assert a[0].sum() == b[0].sum() + (matched == np.uint64(on_matched)).sum() and a[1].sum() > b[1].sum()
    assert (0, 0) in seen and (len(sh), int(_bounded(sh, so, sqh, sqc, 0, 0, 2)[0].sum())) in seen and len(seen) >= 5
    # an empty slice of a truncated sample: the sizes are still counted up to the bound
    d_e, d_ec = held(hip.array(np.zeros(1, np.uint64)), hip.array(np.zeros(1, np.uint32)))
    for make in (lambda: hip.sketch_from_pairs_dev(d_e.ptr, d_ec.ptr, 0, c["k"]),
                 lambda: hip.sketch_merge_dev_async(d_e.ptr, d_ec.ptr, 0, c["k"], lo, hi - 1)):
        empty = held(make())
        for truncated, bound in [(1, on_hash), (1, int(ssh[0]) - 1), (1, U64_MAX), (0, on_hash)]:
            hits, sizes = _run_bounded(hip, empty, table, G, truncated, bound)
            whits, wsizes = _bounded(sh, so, sqh[:0], sqc[:0], truncated, bound, 2)
            assert np.array_equal(sizes, wsizes) and np.array_equal(hits, whits) and not whits.any(), (truncated, bound)
        assert _bounded(sh, so, sqh[:0], sqc[:0], 1, on_hash, 2)[1].sum() not in (0, len(sh))


def test_set_bound_on_a_pending_merge(hip, oracle_lib, bound_case, held):
    """The merge of two ranks' pairs over the whole range, still pending when it is given its bound: it resolves and is right."""
    c = bound_case
    G, dbh, dbo, qh, qc = c["G"], c["dbh"], c["dbo"], c["qh"], c["qc"]
    twice = qc >= 2
    ph = np.concatenate([qh, qh[twice]])
    pc = np.concatenate([np.ones(len(qh), np.uint32), qc[twice] - np.uint32(1)])
    assert len(ph) >= 32768 and c["hmax"] < 2 ** 63
    assert _merge_goes_pending(hip, ph, c["k"], 0, c["hmax"], U64_MAX - 1)
    d_h, d_c = held(hip.array(ph), hip.array(pc))
    table = held(hip.upload_table(dbh, dbo))
    srt = np.sort(dbh)
    for bound in (int(srt[len(srt) // 3]), int(srt[len(srt) // 3]) - 1):
        sk = held(hip.sketch_merge_dev_async(d_h.ptr, d_c.ptr, len(ph), c["k"], 0, c["hmax"]))
        hits, sizes = _run_bounded(hip, sk, table, G, 1, bound)
        whits, wsizes = _bounded(dbh, dbo, qh, qc, 1, bound, 2)
        assert np.array_equal(sizes, wsizes) and np.array_equal(hits, whits) and 0 < wsizes.sum() < len(dbh) and whits.sum() > 0
        assert not sk.resolve()
        gh, gc = sk.download()
        assert np.array_equal(gh, qh) and np.array_equal(gc, qc)


@pytest.mark.parametrize("world", [2, 5])
def test_ranges_of_a_bottom_s_sample_add_up(hip, oracle_lib, bound_case, held, world):
    """The whole path of a truncated sample over W hash ranges: every range's slice of the bottom-s sketch, the table's slice, the
    sample's last hash as the bound of every range — the sums are oracle.containment of the truncated sketch."""
    c = bound_case
    G, k, dbh, dbo = c["G"], c["k"], c["dbh"], c["dbo"]
    b5 = table_bounds(dbh, 5, c["hmax"])
    s = int(np.searchsorted(c["qh"], np.uint64((b5[3] + b5[4]) // 2)))  # the sample ends inside the fourth of five ranges
    qh, qc, truncated, _ = oracle_lib.sketch_reads(c["rb"], c["ro"], k, hmax=c["hmax"], s=s)
    assert truncated and len(qh) == s < len(c["qh"]) and np.array_equal(qh, c["qh"][:s])
    last = int(qh[-1])
    whits, wsizes = oracle_lib.containment(qh, qc, True, 2, dbh, dbo)
    assert 0 < wsizes.sum() < len(dbh) and whits.sum() > 0
    bounds = table_bounds(dbh, world, c["hmax"])
    hits, sizes, empty_slices = np.zeros(G, np.uint64), np.zeros(G, np.uint64), 0
    for r in range(world):
        lo, hi = bounds[r], bounds[r + 1]
        inq = (qh >= np.uint64(lo)) & (qh < np.uint64(hi))
        empty_slices += not inq.any()
        d_h, d_c = held(hip.array(qh[inq] if inq.any() else np.zeros(1, np.uint64)), hip.array(qc[inq] if inq.any() else np.zeros(1, np.uint32)))
        sk = held(hip.sketch_merge_dev(d_h.ptr, d_c.ptr, int(inq.sum()), k, lo, hi - 1))
        sh, so = table_slice(dbh, dbo, lo, hi)
        table = held(hip.upload_table(sh, so))
        hr, sr = _run_bounded(hip, sk, table, G, True, last)
        hits += hr
        sizes += sr
    assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes)
    assert empty_slices == (1 if world == 5 else 0)  # (five ranges: the sample ends before the last of them begins)


# ---------------------------------------------------------------- 4. several k in one launch
@pytest.fixture(scope="module")
def multi_case(hip, oracle_lib):
    """Tables of different k and size — "big": 1100 genomes of a few hashes (counter copies below 64), "tiny": 3 genomes, "other":
    5 genomes at another k, "hollow": 6 genomes whose sketches are all empty (no pair: its tiles are none), "none": no genome —
    and one read set drawn from all the genomes."""
    rng = np.random.default_rng(7600)
    small_b, small_o = random_genomes(rng, 1100, 80)
    large_b, large_o = random_genomes(rng, 8, 2500)
    gb = np.concatenate([small_b, large_b])
    go = np.concatenate([small_o, large_o[1:] + small_o[-1]])
    r1, o1, _ = sample_reads(rng, small_b, small_o, 3000, 60, err=0.01, present=np.arange(0, 1100, 3))
    r2, o2, _ = sample_reads(rng, large_b, large_o, 1500, 150, err=0.01)
    rb, ro = np.concatenate([r1, r2]), np.concatenate([o1, o2[1:] + o1[-1]])
    tabs = {"big": (21, oracle_lib.sketch_genomes(small_b, small_o, 21, 8)),
            "tiny": (31, oracle_lib.sketch_genomes(large_b[: 3 * 2500], large_o[:4], 31, 300)),
            "other": (25, oracle_lib.sketch_genomes(large_b[3 * 2500:], large_o[3:] - large_o[3], 25, 200)),
            "hollow": (51, (np.zeros(0, np.uint64), np.zeros(7, np.uint64))),
            "none": (33, (np.zeros(0, np.uint64), np.zeros(1, np.uint64)))}
    gmax = len(tabs["big"][1][1]) - 1
    copies = 1
    while copies < 64 and copies * 2 * gmax <= 65536:  # (containment_launch's rule)
        copies *= 2
    assert copies < 64 and gmax == 1100
    del gb, go
    d_b, d_o = hip.array(rb), hip.array(ro)
    up = {name: hip.upload_table(h, o) for name, (_, (h, o)) in tabs.items()}
    try:
        assert up["none"].ngenomes == 0 and up["hollow"].ngenomes == 6
        yield dict(tabs=tabs, up=up, rb=rb, ro=ro, d_b=d_b, d_o=d_o, nreads=len(ro) - 1)
    finally:
        for x in list(up.values()) + [d_b, d_o]:
            x.free()


# (sketch, table) of a stage-B call: which sketch goes against which table
_PAIRS = {"big": "pending", "tiny": "truncated", "other": "empty", "hollow": "plain", "none": "plain"}
_S_TRUNCATED = 8000


def _multi_sketches(hip, held, c):
    """Fresh handles: a pending one (its index not built yet), a truncated one (s > 0), an empty one, a plain one."""
    tabs, up = c["tabs"], c["up"]
    d_b, d_o, nreads = c["d_b"], c["d_o"], c["nreads"]
    return {"pending": held(hip.sketch_reads_dev_async(d_b.ptr, d_o.ptr, nreads, tabs["big"][0], up["big"].max_hash, 0)),
            "truncated": held(hip.sketch_reads_dev(d_b.ptr, d_o.ptr, nreads, tabs["tiny"][0], up["tiny"].max_hash, _S_TRUNCATED)),
            "empty": held(hip.sketch_reads_dev(d_b.ptr, d_o.ptr, 0, tabs["other"][0], up["other"].max_hash, 0)),
            "plain": held(hip.sketch_reads_dev(d_b.ptr, d_o.ptr, nreads, 51, U64_MAX // 50, 0))}


@pytest.fixture(scope="module")
def multi_want(oracle_lib, multi_case):
    c = multi_case
    rb, ro, tabs = c["rb"], c["ro"], c["tabs"]
    hm = {name: table_max_hash(*tabs[name][1]) for name in ("big", "tiny")}
    assert rb.size * (hm["big"] + 1) / 2.0 ** 64 >= 1.5 * 32768  # (the counting-table path: the async sketch stays pending)
    q = {"pending": oracle_lib.sketch_reads(rb, ro, tabs["big"][0], hmax=hm["big"])[:3],
         "truncated": oracle_lib.sketch_reads(rb, ro, tabs["tiny"][0], hmax=hm["tiny"], s=_S_TRUNCATED)[:3],
         "empty": (np.zeros(0, np.uint64), np.zeros(0, np.uint32), False),
         "plain": oracle_lib.sketch_reads(rb, ro, 51, hmax=U64_MAX // 50)[:3]}
    assert q["truncated"][2] and not q["pending"][2] and len(q["plain"][0]) > 1000
    assert len(q["pending"][0]) > 2048  # (more distinct hashes than a starved table's sketch holds: _reads_go_pending)
    want = {}
    for name, (_, (h, o)) in tabs.items():
        qh, qc, tr = q[_PAIRS[name]]
        want[name] = oracle_lib.containment(qh, qc, tr, 2, h if len(h) else np.zeros(1, np.uint64), o)
        assert len(want[name][0]) == len(want[name][1]) == len(o) - 1, name  # (one entry per genome; none for "none")
    assert want["big"][0].max() >= 4 and want["tiny"][0].max() > 10 and 0 < want["tiny"][1].max() < 300
    assert want["other"][1].min() == 200 and not want["other"][0].any() and not want["hollow"][1].any()
    return want


def _contain(hip, c, sketches, names, alone):
    """One multi call over `names`, or one containment_dev per name; -> {name: (hits, sizes)}, the guards behind the outputs checked."""
    up = c["up"]
    outs = {name: (hip.array(np.full(up[name].ngenomes + 1, SENT32, np.uint32)), hip.array(np.full(up[name].ngenomes + 1, SENT32, np.uint32)))
            for name in names}
    try:
        if alone:
            for name in names:
                hip.containment_dev(sketches[_PAIRS[name]], up[name], 2, outs[name][0].ptr, outs[name][1].ptr)
        else:
            hip.containment_multi_dev([sketches[_PAIRS[name]] for name in names], [up[name] for name in names], 2,
                                      [outs[name][0].ptr for name in names], [outs[name][1].ptr for name in names])
        hip.sync()
        got = {}
        for name in names:
            g = up[name].ngenomes
            h, s = outs[name][0].download(), outs[name][1].download()
            assert h[g] == SENT32 and s[g] == SENT32, name
            got[name] = (h[:g], s[:g])
        return got
    finally:
        for d_h, d_s in outs.values():
            d_h.free()
            d_s.free()


_LAYOUTS = {"none_first": ["none", "big", "hollow", "tiny"], "none_middle": ["big", "hollow", "none", "tiny"],
            "none_last": ["big", "hollow", "tiny", "none"], "empty_sketch": ["other", "big", "hollow", "tiny"],
            "tiny_first": ["tiny", "other", "big"], "pair": ["hollow", "big"]}


@pytest.mark.parametrize("grid", ["default", "one_workgroup"])
@pytest.mark.parametrize("layout", list(_LAYOUTS))
def test_containment_of_several_k_in_one_launch(hip, multi_case, multi_want, knobs, held, layout, grid):
    c, names = multi_case, _LAYOUTS[layout]
    knobs("distinct_hint_ppm", 1000000)  # (the pending sketch's table sized for every candidate: no rebuild, whatever ran before)
    if "big" in names:
        assert _reads_go_pending(hip, knobs, c["d_b"], c["d_o"], c["nreads"], c["tabs"]["big"][0], c["up"]["big"].max_hash, 0, 1000000)
    if grid == "one_workgroup":
        knobs("kb_grid", 1)  # one workgroup walks every tile of every k
    for first in ("multi", "alone"):  # who builds the index the sketch handle then keeps
        sketches = _multi_sketches(hip, held, c)
        rounds = [("multi", _contain(hip, c, sketches, names, False))]
        if first == "alone":
            rounds.insert(0, ("alone before", _contain(hip, c, sketches, names, True)))
        rounds.append(("alone after", _contain(hip, c, sketches, names, True)))
        for what, got in rounds:
            for name in names:
                assert np.array_equal(got[name][0], multi_want[name][0]), (layout, first, what, name)
                assert np.array_equal(got[name][1], multi_want[name][1]), (layout, first, what, name)
        assert not sketches["pending"].resolve()


def test_containment_of_five_k_is_refused(hip, multi_case, held):
    c = multi_case
    sketches = _multi_sketches(hip, held, c)
    names = ["tiny", "other", "hollow", "none", "tiny"]
    d = held(hip.empty(8, np.uint32))
    with pytest.raises(_hip.HipError):
        hip.containment_multi_dev([sketches[_PAIRS[n]] for n in names], [c["up"][n] for n in names], 2, [d.ptr] * 5, [d.ptr] * 5)


# ---------------------------------------------------------------- 5. a rank's share of the count lists
def test_count_shares_add_up(hip, oracle_lib, count_case, held):
    """Every rank streams its own run of each k < k_max count list (refpipe_count_launch cuts them).  The runs are not looked at
    here, only what they must add up to; a world longer than the shortest list leaves some rank's run of it empty, whatever the cut."""
    table, reads = count_case["table"], count_case["reads"]
    whits, wsizes = count_case["columns"]
    npairs, _, ncount = table.sizes()
    rb, ro = flat(reads)
    d_b, d_o = held(*_reads_dev(hip, rb, ro))
    kc = held(table.kmer_counts())
    kc.add_dev(d_b.ptr, d_o.ptr, len(ro) - 1, int(ro[-1]))
    assert np.array_equal(kc.download(), count_case["want"])
    worlds = (1, 2, 3, 7, 64, min(ncount) + 1)
    assert 64 < min(ncount) < worlds[-1]  # more ranks than the shortest list has entries: a share with an empty run
    assert all(w.any() for w in whits)
    try:
        hits, sizes = hip.refpipe_containment_counts(kc, table, 2)
        assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes)
        for world in worlds:
            total = np.zeros_like(whits[:-1], dtype=np.uint64)
            for rank in range(world):
                table.set_count_share(rank, world)
                hr, sr = hip.refpipe_containment_counts(kc, table, 2)
                assert np.array_equal(hr[-1], whits[-1]) and np.array_equal(sr, wsizes), (world, rank)
                total += hr[:-1]
            assert np.array_equal(total, whits[:-1]), world
        for rank, world in ((0, 0), (3, 3)):
            with pytest.raises(_hip.HipError):
                table.set_count_share(rank, world)
    finally:
        table.set_count_share(0, 1)
    hits, sizes = hip.refpipe_containment_counts(kc, table, 2)
    assert np.array_equal(hits, whits) and np.array_equal(sizes, wsizes)


# ---------------------------------------------------------------- 6. small ones
def test_map_words_of_a_shard(hip, oracle_lib, held):
    """(map[0], map[1], reads) as device words behind the map-only pass, for the first, a middle and the last shard of a stream, with
    and without the lookahead record, and for an empty shard: state_map() / ngroups of a second handle on the same records, the
    sequential restatement of a shard (tests/shard_ref.py), the oracle's read count."""
    rng = np.random.default_rng(7700)
    nref, ntax = 30, 9
    src = rng.integers(0, nref - 1, size=1500)
    recs = synth.make_alignment_records(src + 1, nref)
    ref2tax = rng.integers(0, ntax, size=nref).astype(np.uint32)
    starts = np.flatnonzero(recs["ref_new"] >> 31)
    single = np.diff(np.append(starts, len(recs))) == 1
    fails = single & (recs["matched"][starts] * 2 < recs["total"][starts])
    failing, passing = np.flatnonzero(fails[:-1]), np.flatnonzero(~fails[:-1] & single[:-1])
    after_failing = int(starts[failing[len(failing) // 4] + 1])    # the shard before it ends on an Ambiguous read
    after_passing = int(starts[passing[3 * len(passing) // 4] + 1])
    assert 0 < after_failing < after_passing < len(recs)
    d_r2t = held(hip.array(ref2tax))
    maps = set()
    for a, b in [(0, after_failing), (after_failing, after_passing), (after_passing, len(recs)), (after_failing, after_failing)]:
        for has_look in ([True, False] if b < len(recs) else [False]):
            part = recs[a:b + (1 if has_look else 0)]
            d = held(hip.array(part if len(part) else np.zeros(1, _hip.REC_DTYPE)))
            shard = held(hip.profile_begin_dev(d.ptr, b - a, has_look, d_r2t.ptr, nref, ntax, 0.5))
            d_w = held(hip.array(np.full(4, SENT64, dtype=np.uint64)))
            shard.map_words_dev(d_w.ptr)
            hip.sync()
            w = d_w.download()
            other = held(hip.profile_begin_dev(d.ptr, b - a, has_look, d_r2t.ptr, nref, ntax, 0.5))
            m, groups = other.state_map(), other.ngroups
            assert w[3] == SENT64 and (int(w[0]), int(w[1]), int(w[2])) == (m[0], m[1], groups), (a, b, has_look)
            assert shard.state_map() == m and shard.ngroups == groups
            assert groups == int((recs["ref_new"][a:b] >> 31).sum())
            if b == a:
                assert m == (0, 1) and groups == 0
            else:
                assert groups == oracle_lib.profile_assign(recs[a:b], ref2tax, ntax, 0.5)["tot_rds"]
            if has_look and b > a:
                ref = [shard_ref.run_shard(part, b - a, has_look, ref2tax, ntax, 0.5, x, False, 0) for x in (0, 1)]
                assert (ref[0]["outgoing"], ref[1]["outgoing"]) == m and ref[0]["groups"] == groups, (a, b)
            maps.add(m)
    assert (0, 1) in maps and len(maps) >= 3  # the identity (the empty shard), and shards that end on a kept and on a dropped read


def test_use_resident_switches_between_index_and_bit_filter(hip, oracle_lib, held):
    rng = np.random.default_rng(7800)
    k = 21
    gb, go = random_genomes(rng, 40, 6000)
    dbh, dbo = oracle_lib.sketch_genomes(gb, go, k, 900)
    hmax = table_max_hash(dbh, dbo)
    rb, ro, _ = sample_reads(rng, gb, go, 6000, 150, err=0.01)
    d_b, d_o = held(hip.array(rb), hip.array(ro))
    filt = held(hip.filter_build(dbh))
    assert filt.make_resident(dbh, hmax) and filt.resident_bytes > 0
    fh, fc, _, _ = oracle_lib.sketch_reads_filtered(rb, ro, k, dbh, hmax=hmax)
    uh, uc, _, _ = oracle_lib.sketch_reads(rb, ro, k, hmax=hmax)
    member = np.isin(uh, dbh)
    eh, ec = uh[member], uc[member]
    assert len(fh) > len(eh) > 1000 and np.all(np.isin(eh, fh))  # the bit filter lets hashes through that are not the table's
    for on, (wh, wc) in [(False, (fh, fc)), (True, (eh, ec)), (False, (fh, fc)), (True, (eh, ec))]:
        filt.use_resident(on)
        for fn in (hip.sketch_reads_dev, hip.sketch_reads_dev_async):
            sk = held(fn(d_b.ptr, d_o.ptr, len(ro) - 1, k, hmax, 0, filt=filt))
            h, c = sk.download()
            assert np.array_equal(h, wh) and np.array_equal(c, wc), (on, fn.__name__)
        assert filt.resident_bytes > 0
