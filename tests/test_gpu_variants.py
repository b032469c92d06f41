"""-m gpu: --variants / --variant_sites on the device — the accumulator (mg_variants.hip), the tokenisers' entries and pool
(MG_BATCH_BASES) and the command line.  The expectation is always metalign_amd/variants.py over the same records / lines, and
equality is exact."""
import functools
import gzip

import numpy as np
import pytest

import bamgen
import collate_cases
import identity_cases as ic
import side_bins_cases as sb
import stage_c_checks as sc
import variants_cases as vc
from metalign_amd import _hip
from metalign_amd import collate
from metalign_amd import coverage as cv
from metalign_amd import map_and_profile as mp
from metalign_amd import side_outputs as so
from metalign_amd import side_reads as sr
from metalign_amd import variants as var

pytestmark = pytest.mark.gpu

PCT = 0.5
P = var.Params(5, 2, 50)
# lengths at, below and above the 4096 sites four wavefronts take in one step, a single base, and an accession nobody hits between
# two that are hit
NAMES = ["one", "l4095", "quiet", "l4096", "l4097"]
LENGTHS = [1, 4095, 700, 4096, 4097]
LEN_OF = dict(zip(NAMES, LENGTHS))


def _rec(row, matched=10, total=10, flag=0, new=0):
    return (row | (new << 31), matched, total, flag | (40 << 12))


def _pack(items):
    """[(record, pos0, codes)] (codes None or []: not piled) -> recs, entries, pool."""
    recs = np.array([it[0] for it in items], dtype=_hip.REC_DTYPE) if items else np.zeros(0, dtype=_hip.REC_DTYPE)
    ent, pool = [], bytearray()
    for _, pos0, codes in items:
        ent.append((len(pool), pos0, len(codes)) if codes else (0, 0, 0))
        pool += var.pack(codes or [])
    return recs, (np.array(ent, dtype=_hip.BASES_DTYPE) if ent else np.zeros(0, dtype=_hip.BASES_DTYPE)), bytes(pool)


def _truth(row, pos):
    """The two alleles of a site: every third site has a second one, and so has the last base of every accession."""
    h = (row * 7919 + pos * 104729) & 0xFFFF
    return h & 3, ((h & 3) + 1 + ((h >> 2) % 3)) & 3 if (pos % 3 == 0 or pos in (4094, 4096)) else None


def _generated(n, seed=3):
    """n records: short and long piles around the first and the last base of every accession that is hit (clipped where they go
    past it, unpiled where they start at or behind it), gaps, OTHER bases, records that do not count, rows beyond the accessions."""
    rng = np.random.default_rng(seed)
    rows = [0, 1, 3, 4]
    items = []
    for i in range(n):
        row = rows[int(rng.integers(0, 4))]
        L = LENGTHS[row]
        span = int(rng.choice([1, 2, 3, 3, 8, 40, 151]))
        where = rng.random()
        pos0 = 0 if where < 0.3 else max(0, L - int(rng.integers(1, 4))) if where < 0.7 else int(rng.integers(0, L + 3))
        codes = []
        for j in range(span):
            major, minor = _truth(row, pos0 + j)
            u = rng.random()
            codes.append(5 if u < 0.03 else 4 if u < 0.06 else minor if (minor is not None and u < 0.45) else major)
        kind = i % 17
        if kind == 0:
            items.append((_rec(row, flag=2048), pos0, codes))     # does not count
        elif kind == 1:
            items.append((_rec(row, matched=4), pos0, codes))     # below pct_id
        elif kind == 2:
            items.append((_rec(row, flag=16 | 256, new=1), pos0, None))  # counts, not piled
        elif kind == 3:
            items.append((_rec(int(rng.choice([5, 6, 0x7FFFFFFF]))), pos0, codes))  # a row at or above nacc
        elif kind == 4:
            items.append((_rec(2 if i % 34 == 4 else row), LENGTHS[2 if i % 34 == 4 else row], codes))  # pos0 == L, on `quiet` too
        else:
            items.append((_rec(row, flag=int(rng.choice([0, 16, 256]))), pos0, codes))
    return items


def _check(hip, calls, names=NAMES, lengths=LENGTHS, params=(P,), pct=PCT):
    """The device over `calls` (lists of items, one add_dev each) against the definition over all of them, for every parameter set
    (finish may be called again)."""
    dev = hip.variants(lengths)
    try:
        for items in calls:
            dev.add(*_pack(items), pct)
        got = [dev.result(*p) for p in params]
    finally:
        dev.free()
    recs, ent, pool = _pack([it for items in calls for it in items])
    wants = []
    for p, (aln, call, poly, pairs, disc, unpiled, sites) in zip(params, got):
        want = var.variants_of_records(recs, ent, pool, names, dict(zip(names, lengths)), pct, p)
        per = {a: [int(aln[i]), int(call[i]), int(poly[i]), int(pairs[i]), int(disc[i])] for i, a in enumerate(names) if aln[i]}
        for i, a in enumerate(names):
            if not aln[i]:
                assert (int(call[i]), int(poly[i]), int(pairs[i]), int(disc[i])) == (0, 0, 0, 0)
        assert per == want.per and unpiled == want.unpiled
        assert [(names[int(s["acc"])], int(s["pos0"]), tuple(int(x) for x in s["n"])) for s in sites] == want.sites  # (and their order)
        wants.append(want)
    return wants[0] if len(wants) == 1 else wants


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_add_dev_from_arrays(hip, n):
    want = _check(hip, [_generated(n)])
    if n == 4097:
        assert set(want.per) == {"one", "l4095", "l4096", "l4097"} and want.unpiled > 400 and len(want.sites) > 20
        first_last = {(a, p) for a, p, _ in want.sites}
        for a in ("l4095", "l4096", "l4097"):  # polymorphic sites at the first and the last base of each
            assert (a, 0) in first_last and (a, LEN_OF[a] - 1) in first_last
        assert want.per["one"][1] == 1


def test_identical_records_contend_on_one_site(hip):
    want = _check(hip, [[(_rec(1), 10, [0, 1, 2])] * 4096])
    assert want.per == {"l4095": [4096, 3, 0, 3 * 4096 * 4095, 0]} and want.sites == []


def test_spans_one_two_and_three_behind_one_another(hip):
    """Entries of 1, 1 and 2 bytes: every entry starts on a byte, an odd span leaves a high nibble unused."""
    items = []
    for k in range(6):
        items += [(_rec(3), 5, [k % 4]), (_rec(3), 5, [1, (k + 1) % 4]), (_rec(3), 5, [2, 3, k % 4]), (_rec(3), 4095, [0, 1, 2])]
    want = _check(hip, [items])
    assert want.per["l4096"][0] == 24 and ("l4096", 4095, (6, 0, 0, 0)) not in want.sites and want.per["l4096"][1] == 4
    recs, ent, pool = _pack(items[:4])
    assert ent["off"].tolist() == [0, 1, 2, 4] and len(pool) == 6


def test_a_record_across_the_end_is_clipped_and_one_at_it_is_unpiled(hip):
    items = [(_rec(4), 4095, [0, 0, 1, 1, 1])] * 5 + [(_rec(4), 4097, [2])] * 3 + [(_rec(0), 0, [3, 3, 3])] * 5 + [(_rec(0), 1, [3])]
    want = _check(hip, [items])
    assert want.per == {"l4097": [5, 2, 0, 40, 0], "one": [5, 1, 0, 20, 0]} and want.unpiled == 4


@pytest.mark.parametrize("grid", [1, 2])
def test_the_grid_cut_to_a_few_workgroups(hip, grid):
    _hip.debug_set("var_grid", grid)
    try:
        assert _hip.debug_get("var_grid") == grid
        cut = _check(hip, [_generated(4097, seed=8)])
    finally:
        _hip.debug_set("var_grid", 0)
    assert cut == _check(hip, [_generated(4097, seed=8)]) and len(cut.sites) > 20


@pytest.mark.parametrize("grid", [1, 3])
def test_more_accessions_than_lds_bins_add_to_memory_directly(hip, grid):
    """3000 accessions through the 1024 bins of one workgroup (and of three): at least 1976 of them find no slot, whatever the hash
    does, and add their alignments to memory directly — in the launch that counts the unpiled."""
    assert sb.overflows("mg_variants.hip", "kBins") >= 1000
    rng = np.random.default_rng(12)
    items = [(_rec(row), sb.LENGTH, [1, 2]) if i % 97 == 5 else
             (_rec(row), int(rng.integers(0, 60)), [int(c) for c in rng.integers(0, 4, int(rng.integers(1, 9)))])
             for i, row in enumerate(sb.rows())]
    _hip.debug_set("var_grid", grid)
    try:
        assert _hip.debug_get("var_grid") == grid
        want = _check(hip, [items], names=sb.NAMES, lengths=[sb.LENGTH] * sb.NACC)
    finally:
        _hip.debug_set("var_grid", 0)
    assert len(want.per) > sb.NACC - 70 and want.unpiled >= 2 * len(sb.BEYOND) + 50  # (some accessions' only record is unpiled)


def test_polymorphic_sites_on_both_sides_of_a_step_of_the_block_scan(hip):
    """One accession of 300 000 bases: 293 blocks of 1024 sites for the one workgroup that scans 256 block counts in a step, so the
    sites behind site 256 * 1024 land in their places only with the carry across the step."""
    L, edge = 300000, 256 * 1024
    poly = [5, 1000, 1023, 1024, edge - 1, edge, edge + 7, edge + 1023, edge + 1024, L - 1000, L - 1]
    items = [(_rec(0), p, [k % 2]) for p in poly for k in range(6)]
    items += [(_rec(0), p, [3] * 40) for p in (100, 2000, edge - 200, edge + 5000, L - 300) for _ in range(6)]  # (callable, one allele)
    want = _check(hip, [items], names=["long"], lengths=[L])
    assert [p for _, p, _ in want.sites] == poly and want.per["long"][2] == len(poly) and want.per["long"][1] > len(poly) + 150


def test_a_wavefront_without_bases_between_two_busy_ones_and_lane_63_alone(hip):
    """The four wavefronts of one workgroup: 64 piled records, 64 without a base (unpiled, or not counting), 64 piled ones, and one
    piled record behind 63 without a base."""
    rng = np.random.default_rng(13)

    def busy(n):
        return [(_rec(4), int(rng.integers(0, 4000)), [int(c) for c in rng.integers(0, 4, int(rng.choice([1, 2, 3, 40, 151])))])
                for _ in range(n)]
    idle = [(_rec(4), LENGTHS[4], [1, 2]) if i % 2 else (_rec(4, matched=2), 100, [1, 2, 3]) for i in range(64)]
    items = busy(64) + idle + busy(64) + idle[:63] + [(_rec(4), 4000, [2] * 151)]
    want = _check(hip, [items])
    assert want.per["l4097"][0] == 129 and want.unpiled == 32 + 31
    assert _check(hip, [items[192:]]).per == {"l4097": [1, 0, 0, 0, 0]}


def test_two_and_three_calls_sum_to_one(hip):
    items = _generated(1500, seed=5)
    a = _check(hip, [items])
    b = _check(hip, [items[:700], items[700:]])
    c = _check(hip, [items[:1], items[1:1499], [], items[1499:]])
    assert a == b == c


def test_a_row_at_or_above_nacc_is_unpiled_and_no_accession_is_legal(hip):
    items = [(_rec(0), 0, [1]), (_rec(4), 7, [1, 2]), (_rec(5), 0, [1]), (_rec(0x7FFFFFFF), 0, [1])]
    want = _check(hip, [items])
    assert want.unpiled == 2 and set(want.per) == {"one", "l4097"}
    want = _check(hip, [items], names=[], lengths=[])
    assert want.unpiled == 4 and want.per == {} and want.sites == []
    dev = hip.variants([3, 0, 2])  # (an accession without a base)
    try:
        with pytest.raises(_hip.HipError) as e:
            dev.fetch_sites()
        assert e.value.code == _hip.ERR_STATE
        for bad in ((1, 2, 50), (5, 0, 50), (5, 2, 501)):
            with pytest.raises(_hip.HipError) as e:
                dev.finish(*bad)
            assert e.value.code == _hip.ERR_ARG
        assert dev.finish(5, 2, 50)[5:] == (0, 0) and len(dev.fetch_sites()) == 0
    finally:
        dev.free()


def test_no_polymorphic_site_at_all(hip):
    items = [(_rec(r), p, [c] * 30) for r in (1, 3, 4) for p, c in ((0, 0), (LENGTHS[r] - 30, 2)) for _ in range(6)]
    want = _check(hip, [items])
    assert want.sites == [] and all(st[1:] == [60, 0, 60 * 30, 0] for st in want.per.values())


def test_finish_at_the_threshold_edges_of_the_host_table(hip):
    """Site i of one accession holds SITE_CASES[i]'s four counts; every parameter set of the table judges all of them."""
    items = [(_rec(0), i, [k]) for i, (n4, _, _) in enumerate(vc.SITE_CASES) for k in range(4) for _ in range(n4[k])]
    params = sorted({var.Params(*dcf) for _, dcf, _ in vc.SITE_CASES})
    wants = _check(hip, [items], names=["t"], lengths=[len(vc.SITE_CASES)], params=params)
    for p, want in zip(params, wants):
        for i, (n4, dcf, (ok, major, alleles, pairs, disc)) in enumerate(vc.SITE_CASES):
            if var.Params(*dcf) == p:
                assert (("t", i, tuple(n4)) in want.sites) == bool(alleles), (p, i)
    assert len(params) >= 5 and len({len(w.sites) for w in wants}) > 2


# ---- entries and pool from every tokeniser -------------------------------------------------------------------------------------
def _want_of_lines(lines):
    ent, pool = var.entries_and_pool(f for f in map(cv.retained_fields, lines) if f is not None)
    return np.array(ent, dtype=_hip.BASES_DTYPE), pool


@functools.lru_cache(maxsize=None)
def _case():
    dbinfo, accs, acc2info, taxid2info, acc_index, lines = vc.case(500, 200)
    # reads of five bases: an odd l_seq in the BAM, entries of three bytes
    odd = [ic.L("odd%d" % i, 0, accs[i % 3], cig, ["NM:i:0"], seq=seq).replace("\t1\t60\t", "\t%d\t60\t" % (1000 + i))
           for i, (cig, seq) in enumerate([("5M", "ACGTA"), ("2S3M", "TTACG"), ("2M1I2M", "ACTGT"), ("1M2D2M2S", "NCGTA"), ("5M", "*")] * 3)]
    lines = lines + odd
    return dbinfo, accs, acc2info, taxid2info, acc_index, lines, _want_of_lines(lines)


def _index(hip, acc_index):
    return hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])


def _bases_of(batch):
    try:
        return batch.bases() + (batch.download(),)
    finally:
        batch.free()


def test_hand_table_through_the_tokenisers(hip, tmp_path):
    text = b"".join(ln if isinstance(ln, bytes) else ln.encode() for ln in vc.HAND)
    want_ent, want_pool = _want_of_lines(vc.HAND)
    assert int((want_ent["span"] == 0).sum()) == 5 and want_ent["off"][:3].tolist() == [0, 3, 5]
    idx = _index(hip, vc.ACC_INDEX)
    raw = np.frombuffer(text, dtype=np.uint8)
    d_t = hip.array(raw)
    (tmp_path / "h.sam").write_bytes(text)
    try:
        ent, pool, recs = _bases_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True))
        assert np.array_equal(ent, want_ent) and pool == want_pool and np.array_equal(recs, mp.tokenise_sam(vc.HAND, vc.ACC_INDEX))
        got = hip.sam_tokenize(text, idx, based=True)[-1]
        assert np.array_equal(got[0], want_ent) and got[1] == want_pool
        ent, pool, _ = _bases_of(hip.sam_stream_file(str(tmp_path / "h.sam"), idx, based=True))
        assert np.array_equal(ent, want_ent) and pool == want_pool
        dev = hip.variants([0, 20, 1000, 8])
        try:
            b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True)
            dev.add_batch(b, PCT)
            b.free()
            aln, call, poly, pairs, disc, unpiled, sites = dev.result(*P)
        finally:
            dev.free()
        assert (list(aln), list(call), list(poly), list(pairs), list(disc), unpiled) == ([0, 9, 1, 1], [0, 4, 0, 0], [0, 1, 0, 0],
                                                                                         [0, 122, 0, 0], [0, 72, 0, 0], vc.HAND_UNPILED)
        assert [(int(s["acc"]), int(s["pos0"]), s["n"].tolist()) for s in sites] == [(1, 2, [0, 2, 3, 1])]
    finally:
        d_t.free()
        idx.free()


def _same(a, b):
    """Equality through tuples, lists, dicts and arrays."""
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b and type(a) is type(b)


def _through_add_batch_and_stage_c(hip, tmp_path, batch):
    """Every family's result over `batch`, each fed through SideOutputs.add_batch, then stage C's verdict words and names (which frees
    the batch)."""
    t = lambda name: str(tmp_path / name)
    args = sc.make_args(t("h.sam"), t("db_info.txt"), t("o.cami"), dict(coverage=t("c.tsv"), depth=t("d.tsv"), depth_windows=t("w.tsv"),
                                                                        depth_window_size=4, identity=t("i.tsv"), variants=t("v.tsv")))
    sides = so.SideOutputs.of(args, "h.sam")
    assert sides.families == so.FAMILIES
    try:
        sides.open(hip, dict(zip(vc.ACC_INDEX, [0, 20, 1000, 8])), vc.ACC_INDEX)
        sides.add_batch(batch, PCT)
        out = [dev.result(*(P if fam is so.VARIANTS else ())) for fam, dev in sides._open]
    except BaseException:
        batch.free()
        raise
    finally:
        sides.free()
    res = hip.profile_assign_dev_records(batch.ptr, batch.count, np.arange(4, dtype=np.uint32), 4, PCT, [batch], assign=True)
    return out, res["assign"], res["names"], {k: res[k] for k in ("count", "bases", "first_seen", "tot_rds", "n_ambig")}


@pytest.mark.parametrize("empty", [False, True])
def test_an_uploaded_batch_is_read_as_the_batch_it_was_downloaded_from(hip, tmp_path, empty):
    """The hand table (and a header alone: zero records) tokenised with names, places, edits and bases; everything downloaded and
    uploaded again as an UploadedBatch: the four accumulators and stage C read the two batches alike."""
    text = b"@HD\tVN:1.6\n" if empty else b"".join(ln if isinstance(ln, bytes) else ln.encode() for ln in vc.HAND)
    idx = _index(hip, vc.ACC_INDEX)
    raw = np.frombuffer(text, dtype=np.uint8)
    d_t = hip.array(raw)
    up = None
    try:
        b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, named=True, placed=True, edited=True, based=True)
        try:
            recs, places, edits, bases, names = b.download(), b.places(), b.edits(), b.bases(), b.names()
            assert b.count == (0 if empty else len(mp.tokenise_sam(vc.HAND, vc.ACC_INDEX)))
            up = _hip.UploadedBatch(hip, recs, places=places, edits=edits, bases=bases, names=names)
            assert up.count == b.count and (up.ptr and up.ptr != b.ptr)
        except BaseException:
            b.free()
            raise
        want = _through_add_batch_and_stage_c(hip, tmp_path, b)
        got = _through_add_batch_and_stage_c(hip, tmp_path, up)
        assert _same(got, want)
        if not empty:  # (what the hand table's test holds the accumulator to)
            assert list(want[0][3][0]) == [0, 9, 1, 1] and want[0][3][5] == vc.HAND_UNPILED and len(want[1]) == 2 * (len(names[1]) - 1) > 0
        else:
            assert len(want[1]) == 0 and names[1].tolist() == [0] and int(want[3]["tot_rds"]) == 0
    finally:
        if up is not None:
            up.free()
        d_t.free()
        idx.free()


def test_entries_and_pool_are_the_same_whole_host_streamed_compressed_and_bam(hip, tmp_path):
    _, _, _, _, acc_index, lines, (want_ent, want_pool) = _case()
    text = "".join(lines)
    enc = text.encode()
    assert len(enc) > 3 * (1 << 14) and int((want_ent["span"] == 0).sum()) > 50 and int((want_ent["span"] % 2).sum()) > 10
    assert 4 in var.unpack(want_pool, 2 * len(want_pool)) and 5 in var.unpack(want_pool, 2 * len(want_pool))
    want_recs = mp.tokenise_sam(lines, acc_index)
    idx = _index(hip, acc_index)
    (tmp_path / "n.sam").write_bytes(enc)
    (tmp_path / "n.bgzf.sam.gz").write_bytes(bamgen.bgzf(enc, block=4000, level=0))
    (tmp_path / "n.sam.gz").write_bytes(gzip.compress(enc))
    (tmp_path / "n.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    raw = np.frombuffer(enc, dtype=np.uint8)
    d_t = hip.array(raw)
    got = {}
    try:
        got["whole text"] = _bases_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True))
        got["whole text, placed, edited and named"] = _bases_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True, placed=True,
                                                                                           edited=True, named=True))
        recs, last, (ent, pool) = hip.sam_tokenize(enc, idx, based=True)
        got["host text"] = (ent, pool, recs)
        sam = str(tmp_path / "n.sam")
        # (pieces of 16 KB: at least three of them, so that the second and third pools are moved up behind the ones before)
        got["streamed"] = _bases_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 14, based=True))
        got["streamed, one piece"] = _bases_of(hip.sam_stream_file(sam, idx, based=True))
        got["gzip"] = _bases_of(hip.sam_stream_file(str(tmp_path / "n.sam.gz"), idx, chunk_bytes=1 << 14, based=True))
        got["bgzf, placed"] = _bases_of(hip.sam_stream_file(str(tmp_path / "n.bgzf.sam.gz"), idx, chunk_bytes=1 << 14, based=True, placed=True))
        got["bam"] = _bases_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, chunk_bytes=1 << 13, based=True))
        got["bam, one piece, edited"] = _bases_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, based=True, edited=True))
        _hip.debug_set("stream_thin", 1)  # (a call with the bit never thins its text)
        try:
            got["streamed, thinning on"] = _bases_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 14, based=True))
        finally:
            _hip.debug_set("stream_thin", 0)
        for how, (ent, pool, recs) in got.items():
            assert np.array_equal(recs, want_recs), how
            assert np.array_equal(ent, want_ent), how
            assert pool == want_pool, how
        ent, pool, recs = _bases_of(hip.sam_tokenize_dev_batch(d_t.ptr, 0, idx, based=True))
        assert len(ent) == 0 and len(recs) == 0 and pool == b""
    finally:
        d_t.free()
        idx.free()


def test_a_based_batch_is_collated_with_its_entries_and_the_pool_stays(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case()
    shuffled = collate_cases.coordinate_shuffle("".join(lines))
    text = "".join(shuffled)
    grouped = list(collate.collated_lines(shuffled))
    want_recs = mp.tokenise_sam(grouped, acc_index)
    want_piles = [var.bases_of(f) for f in map(cv.retained_fields, grouped) if f is not None]
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))

    def piles(ent, pool):
        return [(int(e["pos0"]), int(e["span"]), var.unpack(pool[int(e["off"]):int(e["off"]) + (int(e["span"]) + 1) // 2], int(e["span"])))
                for e in ent]
    try:
        b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True, keyed=True)
        try:
            before, pool0 = b.bases()
            perm = b.collate(want_perm=True)
            (after, pool1), recs = b.bases(), b.download()
        finally:
            b.free()
        assert sorted(perm.tolist()) == list(range(len(before))) and not np.array_equal(perm, np.arange(len(perm), dtype=np.uint64))
        assert np.array_equal(after, before[perm.astype(np.int64)]) and pool1 == pool0
        assert np.array_equal(recs, want_recs) and piles(after, pool1) == want_piles
        for how, batch in (("one call", hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, based=True, collate=True)),
                           ("streamed, placed", hip.sam_stream_file(str(tmp_path / "s.sam"), idx, chunk_bytes=1 << 14, based=True, placed=True,
                                                                    collate=True)),
                           ("bam", hip.bam_stream_file(str(tmp_path / "s.bam"), idx, chunk_bytes=1 << 13, based=True, collate=True))):
            ent, pool, recs = _bases_of(batch)
            assert np.array_equal(recs, want_recs) and piles(ent, pool) == want_piles, how
    finally:
        d_t.free()
        idx.free()


def test_paf_is_refused_and_a_plain_batch_has_no_bases(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case()
    text = "".join(lines[:200]).encode()
    (tmp_path / "n.sam").write_bytes(text)
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text, dtype=np.uint8)
    d_t = hip.array(raw)
    try:
        for call in (lambda: hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, paf=True, based=True),
                     lambda: hip.sam_tokenize(text, idx, paf=True, based=True),
                     lambda: hip.sam_stream_file(str(tmp_path / "n.sam"), idx, paf=True, based=True)):
            with pytest.raises(_hip.HipError) as e:
                call()
            assert e.value.code == _hip.ERR_ARG
        for plain in (hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx), hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True,
                                                                                                  edited=True)):
            try:
                for getter in (plain.bases, lambda: plain.bases_ptr, lambda: plain.pool_ptr):
                    with pytest.raises(_hip.HipError) as e:
                        getter()
                    assert e.value.code == _hip.ERR_STATE
            finally:
                plain.free()
    finally:
        d_t.free()
        idx.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
FILES = ("variants", "variant_sites")


def _definitions(d, tag, lines, dbinfo, unique=False, sources=(None,), **params):
    """Both files as the definition gives them: over `lines`, or over side_reads.unique_lines of them."""
    (d / tag).mkdir()
    paths = {k: str(d / tag / (k + ".tsv")) for k in FILES}
    args = sc.make_args("x.sam", dbinfo, "-", dict(paths, **params, **({"side_reads": "unique"} if unique else {})))
    if sources != (None,):
        args.infiles = list(sources)
    acc2info, taxid2info = mp.get_acc2info(args)
    so.write_headers(args)
    feed = (lambda: sr.unique_lines(lines, acc2info, args.pct_id)) if unique else (lambda: lines)
    for src in sources:
        so.SideOutputs.of(args, src or "x.sam").append_from_definition(src or "x.sam", feed, acc2info, taxid2info)
    return {k: open(p, "rb").read() for k, p in paths.items()}


def _run(path, dbinfo, tmp_path, tag, flags=FILES, **extra):
    (tmp_path / tag).mkdir()
    paths = {k: str(tmp_path / tag / (k + ".tsv")) for k in flags}
    out = tmp_path / tag / "out.cami"
    mp.map_main(sc.make_args(str(path), dbinfo, str(out), dict({"input_type": "sam", "db": "unused.fna", "sampleID": "s"}, **paths, **extra)))
    return out.read_bytes(), {k: open(p, "rb").read() for k, p in paths.items()}


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("variants_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = vc.dress(ic.dress(open(sam).read(), 52), 53)
    text = "".join(lines)
    (d / "b.sam").write_text(text)
    (d / "b.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "b.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    return d, [d / "b.sam", d / "b.sam.gz", d / "b.bam"], dbinfo, lines, _definitions(d, "want", lines, dbinfo)


def test_map_main_sam_gz_and_bam_give_the_definitions_bytes(hip, bulk, tmp_path, monkeypatch):
    d, forms, dbinfo, lines, want = bulk
    assert want["variants"].count(b"\nS\t") > 10 and want["variants"].count(b"\nG\t") > 5 and want["variant_sites"].count(b"\n") > 200
    assert int(want["variants"].rsplit(b"\t", 1)[1]) > 100  # (the unpiled)
    cami0, _ = _run(forms[0], dbinfo, tmp_path, "none", flags=())
    for path in forms:
        cami, got = _run(path, dbinfo, tmp_path, "default_" + path.name)
        assert got == want and cami == cami0, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))  # many pieces
        for path in forms:
            assert _run(path, dbinfo, tmp_path, "pieces_" + path.name)[1] == want, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_NO_STREAM", "1")  # the whole text in one tokeniser call
        assert _run(forms[0], dbinfo, tmp_path, "whole")[1] == want
    # either file alone, and other thresholds
    assert _run(forms[0], dbinfo, tmp_path, "sites_alone", flags=("variant_sites",))[1] == {"variant_sites": want["variant_sites"]}
    other = dict(variant_min_depth=3, variant_min_count=1, variant_min_freq=0.2)
    assert _run(forms[2], dbinfo, tmp_path, "other", **other)[1] == _definitions(tmp_path, "want_other", lines, dbinfo, **other)


def test_map_main_with_every_other_side_output(hip, bulk, tmp_path):
    """One tokenisation carries every side array: the variant files are the definition's, the others what they are without them."""
    d, forms, dbinfo, lines, want = bulk
    for path in (forms[0], forms[2]):
        others = {k: str(tmp_path / (path.name + "." + k)) for k in ("coverage", "depth", "identity", "read_assignments")}
        others0 = {k: str(tmp_path / (path.name + ".0." + k)) for k in others}
        cami, got = _run(path, dbinfo, tmp_path, "all_" + path.name, **others)
        cami0, _ = _run(path, dbinfo, tmp_path, "all0_" + path.name, flags=(), **others0)
        assert got == want and cami == cami0, path.name
        for k in others:
            assert open(others[k], "rb").read() == open(others0[k], "rb").read() and len(open(others[k], "rb").read()) > 100, (path.name, k)


def test_map_main_from_uniquely_assigned_reads_only(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, want = bulk
    want_u = _definitions(tmp_path, "want_unique", lines, dbinfo, unique=True)
    assert want_u != want and want_u["variants"].split(b"\n")[2] == b"#reads\tunique"
    for path in (forms[0], forms[2]):
        cov = str(tmp_path / (path.name + ".cov"))
        assert _run(path, dbinfo, tmp_path, "unique_" + path.name, side_reads="unique", coverage=cov)[1] == want_u, path.name


def test_map_main_a_coordinate_sorted_file_with_collate_always(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, _ = bulk
    shuffled = collate_cases.coordinate_shuffle("".join(lines))
    text = "".join(shuffled)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    want = _definitions(tmp_path, "want_sorted", shuffled, dbinfo)
    want_u = _definitions(tmp_path, "want_sorted_unique", list(collate.collated_lines(shuffled)), dbinfo, unique=True)
    for name in ("s.sam", "s.bam"):
        assert _run(tmp_path / name, dbinfo, tmp_path, "sorted_" + name, collate="always")[1] == want, name
    assert _run(tmp_path / "s.sam", dbinfo, tmp_path, "sorted_unique", collate="always", side_reads="unique")[1] == want_u


def test_two_input_files_give_two_blocks(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, _ = bulk
    (tmp_path / "two").mkdir()
    paths = {k: str(tmp_path / "two" / (k + ".tsv")) for k in FILES}
    args = sc.make_args(str(forms[0]), dbinfo, str(tmp_path / "two.cami"), dict({"input_type": "AUTO"}, **paths))
    args.infiles = [str(forms[0]), str(forms[2])]
    mp.map_main(args)
    want = _definitions(tmp_path, "want_two", lines, dbinfo, sources=(str(forms[0]), str(forms[2])))
    assert {k: open(p, "rb").read() for k, p in paths.items()} == want and want["variants"].count(b"#file\t") == 2


def test_the_chunked_path_and_a_chunk_the_host_tokeniser_takes(hip, bulk, tmp_path, monkeypatch):
    """The aligner-stream path (map_and_process over many chunks, their pools joined and their offsets moved up on the host), with a
    chunk that goes through the host tokeniser: FLAG 1_6 is 16 to Python's int() and no number to the device parser, so that chunk's
    entries and pool come from variants.bases_of."""
    d, forms, dbinfo, lines, _ = bulk
    body = [i for i, ln in enumerate(lines) if cv.retained_fields(ln) is not None]
    odd = list(lines)
    for i in (body[len(body) // 2], body[-3]):
        f = odd[i].split("\t")
        f[1] = "1_6"
        odd[i] = "\t".join(f)
    sam = tmp_path / "odd.sam"
    sam.write_text("".join(odd))
    want = _definitions(tmp_path, "want_odd", odd, dbinfo)
    monkeypatch.setattr(mp, "_CHUNK_BYTES", 40000)
    cami, got = _run(sam, dbinfo, tmp_path, "odd", input_type="AUTO", identity=str(tmp_path / "odd.idn"))
    assert got == want
    assert cami == _run(sam, dbinfo, tmp_path, "odd0", flags=(), input_type="AUTO")[0]
    want_u = _definitions(tmp_path, "want_odd_unique", odd, dbinfo, unique=True)
    assert _run(sam, dbinfo, tmp_path, "odd_unique", input_type="AUTO", side_reads="unique")[1] == want_u
