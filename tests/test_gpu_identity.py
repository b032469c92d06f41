"""-m gpu: --identity on the device — the identity kernel (mg_identity.hip), the tokenisers' edits and the command line.  The
expectation is always metalign_amd/identity.py over the same records / lines."""
import ctypes
import functools
import gzip

import numpy as np
import pytest

import bamgen
import collate_cases
import identity_cases as ic
import side_bins_cases as sb
import stage_c_checks as sc
from metalign_amd import _hip
from metalign_amd import bam
from metalign_amd import collate
from metalign_amd import coverage as cv
from metalign_amd import identity as idn
from metalign_amd import map_and_profile as mp

pytestmark = pytest.mark.gpu

PCT = 0.5
GUARD = 0xA5A5A5A5A5A5A5A5
NONE = _hip.EDIT_NONE
NAMES = ["w", "x", "y", "z"]


def _rec(row, matched, total, flag=0, new=0):
    return (row | (new << 31), matched, total, flag | (40 << 12))


def _arrays(pairs):
    recs = np.array([p[0] for p in pairs], dtype=_hip.REC_DTYPE) if pairs else np.zeros(0, dtype=_hip.REC_DTYPE)
    edits = np.array([p[1] for p in pairs], dtype=_hip.EDIT_DTYPE) if pairs else np.zeros(0, dtype=_hip.EDIT_DTYPE)
    return recs, edits


def _edge_pairs():
    """(record, (nm, cols)) pairs on every rule: bins 0 and 1000, nm above cols, no nm, cols 0, the largest values, records that do
    not count, a secondary, every accession row."""
    return [(_rec(0, 10, 10), (0, 150)), (_rec(0, 10, 10), (150, 150)), (_rec(0, 10, 10), (151, 150)), (_rec(0, 10, 10), (NONE, 150)),
            (_rec(0, 10, 10), (3, 0)), (_rec(0, 10, 10), (NONE, 0)), (_rec(1, 10, 10), (1, 1000)), (_rec(1, 10, 10), (1, 1001)),
            (_rec(1, 5, 10), (NONE - 1, NONE)), (_rec(1, 5, 10), (1, NONE)), (_rec(1, 5, 10), (0, NONE)),
            (_rec(2, 4, 10), (0, 100)), (_rec(2, 10, 10, flag=2048), (0, 100)), (_rec(2, 10, 10, flag=256, new=1), (7, 100)),
            (_rec(3, 10, 10, flag=16), (1, 3)), (_rec(3, 10, 10), (2, 3)), (_rec(3, 10, 10), (1, 1))]


def _generated(n, seed=3, nacc=4):
    rng = np.random.default_rng(seed)
    edge = _edge_pairs()
    pairs = []
    for i in range(n):
        if i % 5 == 0:
            pairs.append(edge[(i // 5) % len(edge)])
        else:
            row = int(rng.choice([0, 0, 0, 1, 1, 2, 3])) % nacc
            cols = int(rng.choice([0, 36, 60, 150, 151]))
            nm = int(rng.choice([0, 0, 0, 1, 1, 2, 3, 5, 40, 200, NONE]))
            pairs.append((_rec(row, int(rng.integers(3, 11)), 10, flag=int(rng.choice([0, 16, 256, 2048, 99])), new=int(rng.integers(0, 2))),
                          (nm, cols)))
    return pairs


def _guarded(hip, dev):
    """mg_identity_result and mg_identity_fetch_hist into arrays with guard words behind them."""
    n = dev.nacc
    out = [np.full(n + 4, GUARD, dtype=np.uint64) for _ in range(3)]
    unscored = ctypes.c_uint64(GUARD)
    hip._chk(hip.lib.mg_identity_result(dev.handle, *[_hip._np(a, ctypes.c_uint64) for a in out], ctypes.byref(unscored)))
    for a in out:
        assert np.all(a[n:] == GUARD), "written behind an output array"
    rows = np.arange(n, dtype=np.uint32)
    hist = np.full(n * _hip.IDENTITY_BINS + 4, GUARD, dtype=np.uint64)
    hip._chk(hip.lib.mg_identity_fetch_hist(dev.handle, _hip._np(rows if n else np.zeros(1, np.uint32), ctypes.c_uint32), ctypes.c_uint32(n),
                                            _hip._np(hist, ctypes.c_uint64)))
    assert np.all(hist[n * _hip.IDENTITY_BINS:] == GUARD), "written behind the histogram rows"
    return [a[:n] for a in out], int(unscored.value), hist[:n * _hip.IDENTITY_BINS].reshape(n, _hip.IDENTITY_BINS)


def _check(hip, calls, names=NAMES, pct=PCT):
    """The device over `calls` (lists of pairs, one add_dev each) against the definition over all of them."""
    dev = hip.identity(len(names))
    try:
        for pairs in calls:
            dev.add(*_arrays(pairs), pct)
        (aln, cols, eds), unscored, hist = _guarded(hip, dev)
        again = dev.result()  # (repeatable, and the wrapper's own way to the rows)
    finally:
        dev.free()
    recs, edits = _arrays([p for pairs in calls for p in pairs])
    want = idn.identity_of_records(recs, edits, names, pct)
    got = {}
    for i, a in enumerate(names):
        nz = np.flatnonzero(hist[i])
        if aln[i]:
            got[a] = [int(aln[i]), int(cols[i]), int(eds[i]), dict(zip(nz.tolist(), hist[i][nz].tolist()))]
        else:
            assert int(cols[i]) == 0 and int(eds[i]) == 0 and nz.size == 0
    assert got == want.per
    assert unscored == want.unscored == again[3]
    assert {names[r]: H for r, H in again[4].items()} == {a: st[3] for a, st in want.per.items()}
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_add_dev_from_arrays(hip, n):
    want = _check(hip, [_generated(n)])
    if n == 5000:
        assert set(want.per) == set(NAMES) and want.unscored > 500 and all(len(st[3]) > 5 for st in want.per.values())


def test_every_edge_case_alone_and_together(hip):
    edge = _edge_pairs()
    want = _check(hip, [edge])
    assert want.per["w"] == [3, 450, 300, {1000: 1, 0: 2}] and want.unscored == 3
    # (1, 1000), (1, 1001), (1, 2^32 - 1) -> 999; (2^32 - 2, 2^32 - 1) -> 0; (0, 2^32 - 1) -> 1000
    assert want.per["x"][3] == {999: 3, 0: 1, 1000: 1}
    for p in edge:
        _check(hip, [[p]])


def test_identical_records_contend_on_one_key(hip):
    want = _check(hip, [[(_rec(2, 10, 10), (3, 150))] * 4000])
    assert want.per == {"y": [4000, 600000, 12000, {980: 4000}]} and want.unscored == 0


@pytest.mark.parametrize("grid", [0, 1, 3])
def test_more_keys_than_lds_slots_add_to_memory_directly(hip, grid):
    """40 accessions with identities over all 1001 bins: 40040 keys for the 2048 slots of a workgroup's table (with the grid cut
    to 1 and 3 workgroups, each of them meets thousands)."""
    names = ["a%d" % i for i in range(40)]
    pairs = [(_rec(i % 40, 10, 10), (i // 40, 1000)) for i in range(40 * 1001)]  # nm 0 .. 1000 on every accession: bin 1000 - nm
    pairs += [(_rec(int(r), 10, 10), (int(v), 1000)) for r, v in zip(np.random.default_rng(5).integers(0, 40, 3000),
                                                                     np.random.default_rng(6).integers(0, 1001, 3000))]
    _hip.debug_set("ident_grid", grid)
    try:
        want = _check(hip, [pairs], names=names)
    finally:
        _hip.debug_set("ident_grid", 0)
    assert len(want.per) == 40 and all(len(st[3]) == 1001 for st in want.per.values())


@pytest.mark.parametrize("grid", [1, 3])
def test_more_accessions_than_lds_bins_add_to_memory_directly(hip, grid):
    """3000 accessions through the 512 per-accession bins of one workgroup (and of three): at least 2488 of them find no slot,
    whatever the hash does, and add their three sums to memory directly — in the launch that counts the unscored."""
    assert sb.overflows("mg_identity.hip", "kAccSlots") >= 1000
    rng = np.random.default_rng(12)
    pairs = [(_rec(row, 10, 10), (NONE, 100) if i % 97 == 5 else (int(rng.integers(0, 30)), int(rng.integers(30, 300))))
             for i, row in enumerate(sb.rows())]
    _hip.debug_set("ident_grid", grid)
    try:
        assert _hip.debug_get("ident_grid") == grid
        want = _check(hip, [pairs], names=sb.NAMES)
    finally:
        _hip.debug_set("ident_grid", 0)
    assert len(want.per) > sb.NACC - 70 and want.unscored >= 2 * len(sb.BEYOND) + 50  # (some accessions' only record is unscored)


@pytest.mark.parametrize("grid", [1, 3])
def test_the_grid_cut_to_a_few_workgroups(hip, grid):
    _hip.debug_set("ident_grid", grid)
    try:
        assert _hip.debug_get("ident_grid") == grid
        _check(hip, [_generated(5000, seed=8)])
    finally:
        _hip.debug_set("ident_grid", 0)


def test_two_and_three_calls_sum_to_one(hip):
    pairs = _generated(1500, seed=5)
    a = _check(hip, [pairs])
    b = _check(hip, [pairs[:700], pairs[700:]])
    c = _check(hip, [pairs[:1], pairs[1:1499], [], pairs[1499:]])
    assert a == b == c


def test_a_row_beyond_the_accessions_is_unscored_and_no_accession_is_legal(hip):
    pairs = [(_rec(0, 1, 1), (0, 10)), (_rec(3, 1, 1), (0, 10)), (_rec(4, 1, 1), (0, 10)), (_rec(0x7FFFFFFF, 1, 1), (0, 10))]
    want = _check(hip, [pairs])
    assert want.unscored == 2 and set(want.per) == {"w", "z"}
    want = _check(hip, [pairs], names=[])
    assert want.unscored == 4 and want.per == {}
    dev = hip.identity(2)
    try:
        with pytest.raises(_hip.HipError) as e:
            dev.hist([2])
        assert e.value.code == _hip.ERR_ARG
        assert dev.hist([]).shape == (0, _hip.IDENTITY_BINS)
    finally:
        dev.free()


# ---- edits from every tokeniser -----------------------------------------------------------------------------------------------
def _edits_of_lines(lines):
    kept = [cv.retained_fields(ln) for ln in lines]
    return np.array([idn.edit_of(f) for f in kept if f is not None], dtype=_hip.EDIT_DTYPE)


@functools.lru_cache(maxsize=None)
def _case(bam_safe):
    dbinfo, accs, acc2info, taxid2info, acc_index, lines = ic.case(1200, 500, bam_safe=bam_safe)
    return dbinfo, accs, acc2info, taxid2info, acc_index, lines, _edits_of_lines(lines)


def _index(hip, acc_index):
    return hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])


def _edits_of(batch, placed=False):
    try:
        return (batch.edits(), batch.download()) + ((batch.places(),) if placed else ())
    finally:
        batch.free()


def test_hand_table_through_the_tokenisers(hip, tmp_path):
    acc_index = {"Unmapped": 0, "c1": 1, "c2": 2, "c3": 3, "d1": 4}
    text = b"".join(ln if isinstance(ln, bytes) else ln.encode() for ln in ic.HAND)
    want = _edits_of_lines(ic.HAND)
    assert len(want) == 23 and int((want["nm"] == NONE).sum()) == 7
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text, dtype=np.uint8)
    d_t = hip.array(raw)
    (tmp_path / "h.sam").write_bytes(text)
    try:
        ed, recs = _edits_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True))
        assert np.array_equal(ed, want) and np.array_equal(recs, mp.tokenise_sam(ic.HAND, acc_index))
        assert np.array_equal(hip.sam_tokenize(text, idx, edited=True)[-1], want)
        assert np.array_equal(_edits_of(hip.sam_stream_file(str(tmp_path / "h.sam"), idx, edited=True))[0], want)
        dev = hip.identity(5)
        try:
            b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True)
            dev.add_batch(b, PCT)
            b.free()
            aln, cols, eds, unscored, per = dev.result()
        finally:
            dev.free()
        assert (list(aln), list(cols), list(eds), unscored) == ([0, 7, 2, 0, 4], [0, 160, 30, 0, 38], [0, 24, 19, 0, 5], 7)
        assert per == {1: {1000: 1, 900: 2, 800: 1, 700: 1, 930: 1, 0: 1}, 2: {0: 1, 550: 1}, 4: {900: 1, 1000: 2, 600: 1}}
    finally:
        d_t.free()
        idx.free()


def test_edits_are_the_same_whole_host_streamed_compressed_thinned(hip, tmp_path):
    _, _, _, _, acc_index, lines, want = _case(False)
    text = "".join(lines)
    assert len(text) > 5 * (1 << 16) and int((want["nm"] == NONE).sum()) > 300 and len(np.unique(want["nm"])) > 8
    assert int((want["cols"] == 0).sum()) > 20
    want_recs = mp.tokenise_sam(lines, acc_index)
    want_places = np.array([cv.placement(f) for f in map(cv.retained_fields, lines) if f is not None], dtype=_hip.PLACE_DTYPE)
    assert len(want_recs) == len(want)
    idx = _index(hip, acc_index)
    enc = text.encode()
    (tmp_path / "n.sam").write_bytes(enc)
    (tmp_path / "n.bgzf.sam.gz").write_bytes(bamgen.bgzf(enc, block=4000, level=0))
    (tmp_path / "n.sam.gz").write_bytes(gzip.compress(enc))
    raw = np.frombuffer(enc, dtype=np.uint8)
    d_t = hip.array(raw)
    got = {}
    try:
        got["whole text"] = _edits_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True))
        got["whole text, placed and named"] = _edits_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True, placed=True, named=True),
                                                        placed=True)
        recs, last, ed = hip.sam_tokenize(enc, idx, edited=True)
        got["host text"] = (ed, recs)
        recs, last, nm, pl, ed = hip.sam_tokenize(enc, idx, named=True, placed=True, edited=True)
        got["host text, named and placed"] = (ed, recs, pl)
        sam = str(tmp_path / "n.sam")
        got["streamed"] = _edits_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 12, edited=True))
        got["streamed, placed and named"] = _edits_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 12, edited=True, placed=True, named=True),
                                                      placed=True)
        got["streamed, one piece"] = _edits_of(hip.sam_stream_file(sam, idx, edited=True))
        got["gzip"] = _edits_of(hip.sam_stream_file(str(tmp_path / "n.sam.gz"), idx, chunk_bytes=1 << 12, edited=True))
        got["bgzf"] = _edits_of(hip.sam_stream_file(str(tmp_path / "n.bgzf.sam.gz"), idx, chunk_bytes=1 << 12, edited=True, placed=True),
                                placed=True)
        _hip.debug_set("stream_thin", 1)
        try:
            got["streamed, thinned"] = _edits_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 12, edited=True))
            got["thinned, placed"] = _edits_of(hip.sam_stream_file(sam, idx, chunk_bytes=1 << 14, edited=True, placed=True), placed=True)
        finally:
            _hip.debug_set("stream_thin", 0)
        for how, res in got.items():
            assert np.array_equal(res[0], want), how
            assert np.array_equal(res[1], want_recs), how
            if len(res) > 2:
                assert np.array_equal(res[2], want_places), how
        ed, recs = _edits_of(hip.sam_tokenize_dev_batch(d_t.ptr, 0, idx, edited=True))
        assert len(ed) == 0 and len(recs) == 0
    finally:
        d_t.free()
        idx.free()


def test_edits_from_bam_equal_the_rendering(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case(True)
    text = "".join(lines)
    (tmp_path / "n.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    rendered = list(bam.sam_lines(str(tmp_path / "n.bam")))
    want = _edits_of_lines(rendered)
    # the text and its BAM mean the same, tag for tag: NM of every integer type, of other types, behind every aux type
    assert np.array_equal(want, _edits_of_lines(lines)) and int((want["nm"] == NONE).sum()) > 200
    assert {70000, 300, 2 ** 32 - 2, 77} <= set(want["nm"].tolist())
    for ty in (b":A:", b":f:", b":Z:", b":H:", b":B:c", b":B:C", b":B:s", b":B:S", b":B:i", b":B:I", b":B:f"):
        assert any(ty in ln for ln in rendered), ty
    want_recs = mp.tokenise_sam(lines, acc_index)
    want_places = np.array([cv.placement(f) for f in map(cv.retained_fields, lines) if f is not None], dtype=_hip.PLACE_DTYPE)
    idx = _index(hip, acc_index)
    try:
        got = {"bam": _edits_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, chunk_bytes=1 << 12, edited=True)),
               "bam, one piece": _edits_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, edited=True)),
               "bam, placed and named": _edits_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, chunk_bytes=1 << 12, edited=True, placed=True,
                                                                      named=True), placed=True)}
        stream, hdr, names = bamgen.encode(text)
        body = np.frombuffer(stream[hdr:], dtype=np.uint8)
        d_b = hip.array(body)
        try:
            refmap = [acc_index.get(n, -1) for n in names]
            b, used = hip.bam_tokenize_dev(d_b.ptr, body.size, refmap, idx, edited=True)
            assert used == body.size
            got["records in HBM"] = _edits_of(b)
        finally:
            d_b.free()
        for how, res in got.items():
            assert np.array_equal(res[0], want), how
            assert np.array_equal(res[1], want_recs), how
            if len(res) > 2:
                assert np.array_equal(res[2], want_places), how
    finally:
        idx.free()


def test_an_edited_batch_is_collated_with_its_edits(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case(True)
    shuffled = collate_cases.coordinate_shuffle("".join(lines[:2500]))
    text = "".join(shuffled)
    grouped = list(collate.collated_lines(shuffled))
    want_recs = mp.tokenise_sam(grouped, acc_index)
    want_edits = _edits_of_lines(grouped)
    want_places = np.array([cv.placement(f) for f in map(cv.retained_fields, grouped) if f is not None], dtype=_hip.PLACE_DTYPE)
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    (tmp_path / "s.sam.gz").write_bytes(gzip.compress(text.encode()))
    try:
        b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True, keyed=True)
        try:
            before = b.edits()
            perm = b.collate(want_perm=True)
            after, recs = b.edits(), b.download()
        finally:
            b.free()
        assert sorted(perm.tolist()) == list(range(len(before))) and not np.array_equal(perm, np.arange(len(perm), dtype=np.uint64))
        assert np.array_equal(after, before[perm.astype(np.int64)]) and not np.array_equal(after, before)
        assert np.array_equal(recs, want_recs) and np.array_equal(after, want_edits)
        for how, batch in (("one call", hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True, collate=True)),
                           ("one call, placed", hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True, placed=True, collate=True)),
                           ("streamed", hip.sam_stream_file(str(tmp_path / "s.sam"), idx, chunk_bytes=1 << 12, edited=True, collate=True)),
                           ("gzip, placed", hip.sam_stream_file(str(tmp_path / "s.sam.gz"), idx, chunk_bytes=1 << 12, edited=True, placed=True,
                                                                collate=True)),
                           ("bam", hip.bam_stream_file(str(tmp_path / "s.bam"), idx, chunk_bytes=1 << 12, edited=True, collate=True))):
            res = _edits_of(batch, placed="placed" in how)
            assert np.array_equal(res[1], want_recs) and np.array_equal(res[0], want_edits), how
            if len(res) > 2:
                assert np.array_equal(res[2], want_places), how
    finally:
        d_t.free()
        idx.free()


def test_paf_is_refused_and_a_plain_batch_has_no_edits(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case(True)
    text = "".join(lines[:200]).encode()
    (tmp_path / "n.sam").write_bytes(text)
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text, dtype=np.uint8)
    d_t = hip.array(raw)
    try:
        for call in (lambda: hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, paf=True, edited=True),
                     lambda: hip.sam_tokenize(text, idx, paf=True, edited=True),
                     lambda: hip.sam_stream_file(str(tmp_path / "n.sam"), idx, paf=True, edited=True)):
            with pytest.raises(_hip.HipError) as e:
                call()
            assert e.value.code == _hip.ERR_ARG
        with pytest.raises(_hip.HipError) as e:
            hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, edited=True, named=True, collate=True)
        assert e.value.code == _hip.ERR_STATE
        for plain in (hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx), hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True)):
            try:
                with pytest.raises(_hip.HipError) as e:
                    plain.edits()
                assert e.value.code == _hip.ERR_STATE
                with pytest.raises(_hip.HipError) as e:
                    plain.edits_ptr
                assert e.value.code == _hip.ERR_STATE
            finally:
                plain.free()
    finally:
        d_t.free()
        idx.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _definition_bytes(lines, dbinfo_path, pct_id=0.5, source=None, header=True):
    acc2info, taxid2info = mp.get_acc2info(sc.make_args("-", dbinfo_path, "-", {}))
    got = idn.identity(lines, acc2info, pct_id)
    return ((idn.HEADER if header else "") + idn.format_block(idn.rows(got, acc2info, taxid2info), got.unscored, source)).encode()


def _run(sam, dbinfo, tmp_path, tag, identity=True, **extra):
    out, tsv = tmp_path / (tag + ".cami"), tmp_path / (tag + ".identity.tsv")
    ov = dict({"input_type": "AUTO", "sampleID": "s"}, **extra)
    if identity:
        ov["identity"] = str(tsv)
    mp.map_main(sc.make_args(str(sam), str(dbinfo), str(out), ov))
    return out.read_text(), (tsv.read_bytes() if tsv.exists() else None)


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("identity_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = ic.dress(open(sam).read(), 52)
    text = "".join(lines)
    (d / "b.sam").write_text(text)
    (d / "b.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "b.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    return d, [d / "b.sam", d / "b.sam.gz", d / "b.bam"], dbinfo, lines, _definition_bytes(lines, dbinfo)


def test_map_main_sam_gz_and_bam_give_the_definitions_bytes(hip, bulk, tmp_path, monkeypatch):
    d, forms, dbinfo, lines, want = bulk
    assert want.count(b"\nS\t") > 10 and want.count(b"\nG\t") > 5 and int(want.rsplit(b"\t", 1)[1]) > 100
    kw = dict(input_type="sam", db="unused.fna")
    for path in forms:
        cami, got = _run(path, dbinfo, tmp_path, "default", **kw)
        cami0, none = _run(path, dbinfo, tmp_path, "default_0", identity=False, **kw)
        assert got == want and none is None and cami == cami0, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))  # many pieces
        for path in forms:
            assert _run(path, dbinfo, tmp_path, "pieces", **kw)[1] == want, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_NO_STREAM", "1")  # the whole text in one tokeniser call
        assert _run(forms[0], dbinfo, tmp_path, "whole", **kw)[1] == want


def test_map_main_with_coverage_depth_and_read_assignments(hip, bulk, tmp_path):
    """One tokenisation carries every side array: the identity file is the definition's, and the three other files are what they
    are without --identity."""
    d, forms, dbinfo, lines, want = bulk
    for path in forms:
        files = {k: tmp_path / (path.name + "." + k) for k in ("coverage", "depth", "depth_windows", "read_assignments")}
        files0 = {k: tmp_path / (path.name + ".0." + k) for k in files}
        kw = dict(input_type="sam", db="unused.fna", depth_window_size=500)
        cami, got = _run(path, dbinfo, tmp_path, "all", **kw, **{k: str(p) for k, p in files.items()})
        cami0, none = _run(path, dbinfo, tmp_path, "all_0", identity=False, **kw, **{k: str(p) for k, p in files0.items()})
        assert got == want and none is None and cami == cami0, path.name
        for k in files:
            assert files[k].read_bytes() == files0[k].read_bytes() and files[k].stat().st_size > 100, (path.name, k)


def test_map_main_a_coordinate_sorted_file_with_collate_auto(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, _ = bulk
    head = ["@HD\tVN:1.6\tSO:unsorted\n"] + [ln for ln in lines if ln.startswith("@") and not ln.startswith("@HD")]
    shuffled = collate_cases.coordinate_shuffle("".join(head + [ln for ln in lines if not ln.startswith("@")]))
    assert shuffled[0].startswith("@HD") and "SO:coordinate" in shuffled[0]
    want = _definition_bytes(shuffled, dbinfo)
    text = "".join(shuffled)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    for name in ("s.sam", "s.bam"):
        cov = tmp_path / (name + ".cov")
        cami, got = _run(tmp_path / name, dbinfo, tmp_path, "auto", input_type="sam", db="unused.fna", collate="auto", coverage=str(cov))
        cami0, _ = _run(tmp_path / name, dbinfo, tmp_path, "auto_0", identity=False, input_type="sam", db="unused.fna", collate="auto")
        assert got == want and cami == cami0 and cov.stat().st_size > 100, name


def test_two_input_files_give_two_blocks(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, want = bulk
    out, tsv = tmp_path / "two.cami", tmp_path / "two.tsv"
    args = sc.make_args(str(forms[0]), str(dbinfo), str(out), {"input_type": "AUTO", "identity": str(tsv)})
    args.infiles = [str(forms[0]), str(forms[2])]
    mp.map_main(args)
    assert tsv.read_bytes() == (_definition_bytes(lines, dbinfo, source=str(forms[0]))
                                + _definition_bytes(lines, dbinfo, source=str(forms[2]), header=False))


def test_the_chunked_path_and_a_chunk_the_host_tokeniser_takes(hip, bulk, tmp_path, monkeypatch):
    """The aligner-stream path (map_and_process over many chunks), with a chunk that goes through the host tokeniser: FLAG 1_6 is
    16 to Python's int() and no number to the device parser, so that chunk's edits come from identity.edit_of."""
    d, forms, dbinfo, lines, _ = bulk
    body = [i for i, ln in enumerate(lines) if cv.retained_fields(ln) is not None]
    odd = list(lines)
    for i in (body[len(body) // 2], body[-3]):
        f = odd[i].split("\t")
        f[1] = "1_6"
        odd[i] = "\t".join(f)
    sam = tmp_path / "odd.sam"
    sam.write_text("".join(odd))
    want = _definition_bytes(odd, dbinfo)
    monkeypatch.setattr(mp, "_CHUNK_BYTES", 40000)
    cov = tmp_path / "odd.cov"
    cami, got = _run(sam, dbinfo, tmp_path, "odd", coverage=str(cov))
    assert got == want and cov.stat().st_size > 100
    assert cami == _run(sam, dbinfo, tmp_path, "odd0", identity=False)[0]
    # ... and identity alone on that path
    assert _run(sam, dbinfo, tmp_path, "odd1")[1] == want
