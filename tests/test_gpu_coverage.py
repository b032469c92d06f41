"""-m gpu: --coverage on the device — the coverage kernels (mg_coverage.hip), the placed tokenisers and the command line.  The
expectation is always metalign_amd/coverage.py over the same records / lines."""
import ctypes
import functools
import gzip
import os

import numpy as np
import pytest

import bamgen
import collate_cases
import coverage_cases as cc
import side_bins_cases as sb
import stage_c_checks as sc
from metalign_amd import _hip
from metalign_amd import collate
from metalign_amd import coverage as cv
from metalign_amd import map_and_profile as mp

pytestmark = pytest.mark.gpu

PCT = 0.5
GUARD = 0xA5A5A5A5A5A5A5A5
NAMES = ["a1", "a31", "a33", "big", "huge"]
LENGTHS = {"a1": 1, "a31": 31, "a33": 33, "big": 100000, "huge": 3 << 20}


def _rec(row, matched, total, flag=0, new=0):
    return (row | (new << 31), matched, total, flag | (40 << 12))


def _edge_pairs():
    """(record, place) pairs that start and end on every word edge, stop at L, run past it, sit on L - 1 and on L, do not count."""
    out = []
    big, L = 3, LENGTHS["big"]
    for b in (0, 31, 32, 63, 64):
        for e in (1, 31, 32, 33, 63, 64, 65, 96, 97):
            if e > b:
                out.append((_rec(big, 9, 10), (b, e - b)))
    out += [(_rec(big, 5, 10), (L - 40, 40)), (_rec(big, 5, 10), (L - 40, 41)), (_rec(big, 5, 10), (L - 7, 4000)),  # at L, past L
            (_rec(big, 5, 10), (L - 1, 1)), (_rec(big, 5, 10), (L - 1, 50)), (_rec(big, 5, 10), (L, 10)),         # L - 1, and L: unplaced
            (_rec(big, 5, 10), (1000, 0)),                                                                        # span 0: unplaced
            (_rec(big, 4, 10), (2000, 10)), (_rec(big, 10, 10, flag=2048), (2000, 10)),                           # do not count
            (_rec(big, 10, 10, flag=256, new=1), (3000, 10)),                                                     # a secondary counts
            (_rec(0, 1, 1), (0, 1)), (_rec(0, 1, 1), (0, 40)), (_rec(0, 1, 1), (1, 1)),
            (_rec(1, 1, 1), (0, 31)), (_rec(1, 1, 1), (30, 5)), (_rec(1, 1, 1), (31, 1)), (_rec(1, 1, 1), (3, 4)),
            (_rec(2, 1, 1), (0, 33)), (_rec(2, 1, 1), (31, 2)), (_rec(2, 1, 1), (32, 1)), (_rec(2, 1, 1), (33, 1)),
            (_rec(2, 1, 1), (5, 2 ** 32 - 1))]
    return out


def _arrays(pairs):
    recs = np.array([p[0] for p in pairs], dtype=_hip.REC_DTYPE) if pairs else np.zeros(0, dtype=_hip.REC_DTYPE)
    places = np.array([p[1] for p in pairs], dtype=_hip.PLACE_DTYPE) if pairs else np.zeros(0, dtype=_hip.PLACE_DTYPE)
    return recs, places


def _generated(n, seed=3):
    rng = np.random.default_rng(seed)
    edge = _edge_pairs()
    pairs = []
    for i in range(n):
        if i % 3 == 0:
            pairs.append(edge[(i // 3) % len(edge)])
        else:
            row = int(rng.integers(0, 4))
            L = LENGTHS[NAMES[row]]
            pairs.append((_rec(row, int(rng.integers(3, 11)), 10, flag=int(rng.choice([0, 16, 256, 2048, 99])), new=int(rng.integers(0, 2))),
                          (int(rng.integers(0, L + 3)), int(rng.choice([0, 1, 31, 32, 33, 40, 150, 5000])))))
    return pairs


def _guarded_result(hip, dev):
    """mg_coverage_result into arrays with guard words behind them."""
    n = dev.nacc
    out = [np.full(n + 4, GUARD, dtype=np.uint64) for _ in range(3)]
    unplaced = ctypes.c_uint64(GUARD)
    hip._chk(hip.lib.mg_coverage_result(dev.handle, *[_hip._np(a, ctypes.c_uint64) for a in out], ctypes.byref(unplaced)))
    for a in out:
        assert np.all(a[n:] == GUARD), "written behind an output array"
    return [a[:n] for a in out], int(unplaced.value)


def _check(hip, calls, names=NAMES, pct=PCT, lengths=LENGTHS):
    """The device over `calls` (lists of pairs, one add_dev each) against the definition over all of them."""
    lengths = {a: lengths[a] for a in names}
    dev = hip.coverage([lengths[a] for a in names])
    try:
        for pairs in calls:
            dev.add(*_arrays(pairs), pct)
        (aln, bases, covered), unplaced = _guarded_result(hip, dev)
    finally:
        dev.free()
    recs, places = _arrays([p for pairs in calls for p in pairs])
    want = cv.coverage_of_records(recs, places, names, lengths, pct)
    got = {a: [int(aln[i]), int(bases[i]), int(covered[i])] for i, a in enumerate(names) if aln[i]}
    assert got == want.per
    assert all(int(bases[i]) == 0 and int(covered[i]) == 0 for i in range(len(names)) if not aln[i])
    assert unplaced == want.unplaced
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_add_dev_from_arrays(hip, n):
    want = _check(hip, [_generated(n)], names=NAMES[:4])
    if n == 4097:
        assert set(want.per) == set(NAMES[:4]) and want.unplaced > 100
        assert want.per["a1"][2] == 1 and want.per["a31"][2] == 31 and want.per["a33"][2] == 33


def test_every_edge_case_alone_and_together(hip):
    edge = _edge_pairs()
    _check(hip, [edge], names=NAMES[:4])
    for p in edge:
        _check(hip, [[p]], names=NAMES[:4])


def test_identical_intervals_contend_on_one_word_and_one_accession(hip):
    want = _check(hip, [[(_rec(3, 10, 10), (1234, 20))] * 2000], names=NAMES[:4])
    assert want.per == {"big": [2000, 40000, 20]}


@pytest.mark.parametrize("grid", [0, 2])
def test_one_long_alignment_among_short_ones(hip, grid):
    rng = np.random.default_rng(9)
    pairs = [(_rec(4, 10, 10), (int(p), 40)) for p in rng.integers(0, LENGTHS["huge"] - 40, 4000)]
    pairs.insert(1777, (_rec(4, 10, 10), (12345, 1 << 20)))
    pairs += _generated(300)
    _hip.debug_set("cov_grid", grid)
    try:
        want = _check(hip, [pairs])
    finally:
        _hip.debug_set("cov_grid", 0)
    assert want.per["huge"][0] == 4001 and want.per["huge"][2] > (1 << 20)


@pytest.mark.parametrize("grid", [1, 3])
def test_more_accessions_than_lds_bins_add_to_memory_directly(hip, grid):
    """3000 accessions through the 1024 bins of one workgroup (and of three): at least 1976 of them find no slot, whatever the hash
    does, and add their alignments and bases to memory directly — in the launch that counts the unplaced."""
    assert sb.overflows("mg_coverage.hip", "kCovBins") >= 1000
    rng = np.random.default_rng(12)
    pairs = [(_rec(row, 10, 10), (sb.LENGTH, 9) if i % 97 == 5 else (int(rng.integers(0, 60)), int(rng.integers(1, 40))))
             for i, row in enumerate(sb.rows())]
    _hip.debug_set("cov_grid", grid)
    try:
        assert _hip.debug_get("cov_grid") == grid
        want = _check(hip, [pairs], names=sb.NAMES, lengths=dict.fromkeys(sb.NAMES, sb.LENGTH))
    finally:
        _hip.debug_set("cov_grid", 0)
    assert len(want.per) > sb.NACC - 70 and want.unplaced >= 2 * len(sb.BEYOND) + 50  # (some accessions' only record is unplaced)


def test_a_wavefront_without_words_between_two_busy_ones_and_lane_63_alone(hip):
    """The four wavefronts of one workgroup: 64 placed records, 64 without a word (unplaced, or not counting), 64 placed ones, and
    one placed record behind 63 without a word."""
    rng = np.random.default_rng(13)
    big = 3

    def busy(n):
        return [(_rec(big, 10, 10), (int(rng.integers(0, 90000)), int(rng.choice([1, 31, 33, 150, 5000])))) for _ in range(n)]
    idle = [(_rec(big, 10, 10), (LENGTHS["big"], 5)) if i % 2 else (_rec(big, 2, 10), (100, 50)) for i in range(64)]
    pairs = busy(64) + idle + busy(64) + idle[:63] + [(_rec(big, 10, 10), (70000, 2000))]
    want = _check(hip, [pairs], names=NAMES[:4])
    assert want.per["big"][0] == 129 and want.unplaced == 32 + 31
    assert _check(hip, [pairs[192:]], names=NAMES[:4]).per == {"big": [1, 2000, 2000]}


def test_two_calls_sum_to_one(hip):
    pairs = _generated(1500, seed=5)
    a = _check(hip, [pairs])
    b = _check(hip, [pairs[:700], pairs[700:], []])
    assert a.per == b.per and a.unplaced == b.unplaced


def test_no_accession_and_empty_accessions(hip):
    dev = hip.coverage([])
    try:
        assert dev.result()[3] == 0
    finally:
        dev.free()
    dev = hip.coverage([0, 0, 5, 0])
    try:
        dev.add(*_arrays([(_rec(0, 1, 1), (0, 1)), (_rec(2, 1, 1), (4, 9)), (_rec(3, 1, 1), (0, 1)), (_rec(9, 1, 1), (0, 1))]), PCT)
        aln, bases, covered, unplaced = dev.result()
        assert list(aln) == [0, 0, 1, 0] and list(bases) == [0, 0, 1, 0] and list(covered) == [0, 0, 1, 0] and unplaced == 3
    finally:
        dev.free()


def test_bit_offsets_beyond_32_bits(hip):
    """Three accessions of 2^31 - 1 bases (an 805 MB bitmap): the third one's bits lie beyond bit 2^32."""
    L = 2 ** 31 - 1
    names = ["x", "y", "z"]
    lengths = dict.fromkeys(names, L)
    rng = np.random.default_rng(4)
    pairs = []
    for row in range(3):
        for _ in range(12):
            pairs.append((_rec(row, 10, 10), (int(L - 1 - rng.integers(0, 1000)), int(rng.integers(1, 300)))))
        pairs.append((_rec(row, 10, 10), (L - 1, 7)))
        pairs.append((_rec(row, 10, 10), (0, 33 + row)))
    recs, places = _arrays(pairs)
    want = cv.coverage_of_records(recs, places, names, lengths, PCT)
    dev = hip.coverage([L] * 3)
    try:
        dev.add(recs, places, PCT)
        aln, bases, covered, unplaced = dev.result()
    finally:
        dev.free()
        hip.mem_trim()
    assert {a: [int(aln[i]), int(bases[i]), int(covered[i])] for i, a in enumerate(names)} == want.per
    assert unplaced == want.unplaced == 0 and all(want.per[a][2] > 900 for a in names)


# ---- places from every tokeniser ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    dbinfo, accs, acc2info, taxid2info, acc_index, lines = cc.case(1200, 500)
    kept = [cv.retained_fields(ln) for ln in lines]
    want = np.array([cv.placement(f) for f in kept if f is not None], dtype=_hip.PLACE_DTYPE)
    return dbinfo, accs, acc2info, taxid2info, acc_index, lines, want


def _index(hip, acc_index):
    return hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])


def _places_of(batch):
    try:
        return batch.places(), batch.download()
    finally:
        batch.free()


def test_places_are_the_same_whole_host_streamed_bgzf_and_bam(hip, tmp_path):
    _, _, _, _, acc_index, lines, want = _case()
    text = "".join(lines)
    assert len(text) > 5 * (1 << 16) and int((want["span"] == 0).sum()) > 50 and len(np.unique(want["pos0"])) > 1000
    want_recs = mp.tokenise_sam(lines, acc_index)
    assert len(want_recs) == len(want)
    idx = _index(hip, acc_index)
    (tmp_path / "n.sam").write_text(text)
    (tmp_path / "n.sam.gz").write_bytes(bamgen.bgzf(text.encode(), block=4000, level=0))
    (tmp_path / "n.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    got = {}
    try:
        got["whole text"] = _places_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True))
        recs, last, pl = hip.sam_tokenize(text.encode(), idx, placed=True)
        got["host text"] = (pl, recs)
        recs, last, nm, pl = hip.sam_tokenize(text.encode(), idx, named=True, placed=True)
        got["host text, named"] = (pl, recs)
        got["streamed"] = _places_of(hip.sam_stream_file(str(tmp_path / "n.sam"), idx, chunk_bytes=1 << 12, placed=True))
        got["streamed, named"] = _places_of(hip.sam_stream_file(str(tmp_path / "n.sam"), idx, chunk_bytes=1 << 12, placed=True, named=True))
        got["bgzf"] = _places_of(hip.sam_stream_file(str(tmp_path / "n.sam.gz"), idx, chunk_bytes=1 << 12, placed=True))
        got["bam"] = _places_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, chunk_bytes=1 << 12, placed=True))
        got["bam, one piece"] = _places_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, placed=True))
        _hip.debug_set("stream_thin", 1)
        try:
            got["streamed, thinned"] = _places_of(hip.sam_stream_file(str(tmp_path / "n.sam"), idx, chunk_bytes=1 << 12, placed=True))
        finally:
            _hip.debug_set("stream_thin", 0)
        for how, (pl, recs) in got.items():
            assert np.array_equal(pl, want), how
            assert np.array_equal(recs, want_recs), how
        plain = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx)
        with pytest.raises(_hip.HipError) as e:
            plain.places()
        assert e.value.code == _hip.ERR_STATE
        plain.free()
        with pytest.raises(_hip.HipError) as e:
            hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, paf=True, placed=True)
        assert e.value.code == _hip.ERR_ARG
        with pytest.raises(_hip.HipError) as e:
            hip.sam_stream_file(str(tmp_path / "n.sam"), idx, paf=True, placed=True)
        assert e.value.code == _hip.ERR_ARG
        with pytest.raises(_hip.HipError) as e:
            hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True, named=True, collate=True)
        assert e.value.code == _hip.ERR_STATE
        pl, recs = _places_of(hip.sam_tokenize_dev_batch(d_t.ptr, 0, idx, placed=True))
        assert len(pl) == 0 and len(recs) == 0
    finally:
        d_t.free()
        idx.free()


def test_a_placed_batch_is_collated_with_its_places(hip, tmp_path):
    _, _, _, _, acc_index, lines, _ = _case()
    shuffled = collate_cases.coordinate_shuffle("".join(lines[:2500]))
    text = "".join(shuffled)
    want_recs = mp.tokenise_sam(collate.collated_lines(shuffled), acc_index)
    want_places = np.array([cv.placement(f) for f in map(cv.retained_fields, collate.collated_lines(shuffled)) if f is not None],
                           dtype=_hip.PLACE_DTYPE)
    idx = _index(hip, acc_index)
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    (tmp_path / "s.sam.gz").write_bytes(bamgen.bgzf(text.encode(), block=4000, level=0))
    (tmp_path / "s.gzip.sam.gz").write_bytes(gzip.compress(text.encode()))
    try:
        b = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True, keyed=True)
        try:
            before = b.places()
            perm = b.collate(want_perm=True)
            after, recs = b.places(), b.download()
        finally:
            b.free()
        assert sorted(perm.tolist()) == list(range(len(before))) and not np.array_equal(perm, np.arange(len(perm), dtype=np.uint64))
        assert np.array_equal(after, before[perm.astype(np.int64)])
        assert np.array_equal(recs, want_recs) and np.array_equal(after, want_places)
        for how, batch in (("one call", hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, placed=True, collate=True)),
                           ("streamed", hip.sam_stream_file(str(tmp_path / "s.sam"), idx, chunk_bytes=1 << 12, placed=True, collate=True)),
                           ("bgzf", hip.sam_stream_file(str(tmp_path / "s.sam.gz"), idx, chunk_bytes=1 << 12, placed=True, collate=True)),
                           ("gzip", hip.sam_stream_file(str(tmp_path / "s.gzip.sam.gz"), idx, chunk_bytes=1 << 12, placed=True, collate=True)),
                           ("bam", hip.bam_stream_file(str(tmp_path / "s.bam"), idx, chunk_bytes=1 << 12, placed=True, collate=True))):
            pl, recs = _places_of(batch)
            assert np.array_equal(recs, want_recs) and np.array_equal(pl, want_places), how
    finally:
        d_t.free()
        idx.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _definition_bytes(lines, dbinfo_path, pct_id=0.5, source=None, header=True):
    acc2info, taxid2info = mp.get_acc2info(sc.make_args("-", dbinfo_path, "-", {}))
    got = cv.coverage(lines, acc2info, pct_id)
    return ((cv.HEADER if header else "") + cv.format_block(cv.rows(got, acc2info, taxid2info), got.unplaced, source)).encode()


def _run(sam, dbinfo, tmp_path, tag, **extra):
    out, cov = tmp_path / (tag + ".cami"), tmp_path / (tag + ".cov.tsv")
    ov = dict({"input_type": "AUTO", "sampleID": "s"}, **extra)
    if ov.pop("cov", True):
        ov["coverage"] = str(cov)
    mp.map_main(sc.make_args(str(sam), str(dbinfo), str(out), ov))
    return out.read_text(), (cov.read_bytes() if cov.exists() else None)


def _dressed(sam_path, dbinfo_path, seed):
    acc2info, _ = cc.tables(open(dbinfo_path).read())
    accs = [a for a in acc2info if a != "Unmapped"]
    return cc.dress(open(sam_path).read(), accs, acc2info, seed)


def _three_forms(d, stem, lines):
    text = "".join(lines)
    (d / (stem + ".sam")).write_text(text)
    (d / (stem + ".sam.gz")).write_bytes(gzip.compress(text.encode()))
    (d / (stem + ".bam")).write_bytes(bamgen.sam_to_bam(text, block=20000))
    return [d / (stem + ".sam"), d / (stem + ".sam.gz"), d / (stem + ".bam")]


def _chunked(path, dbinfo, tmp_path, tag):
    """The file's lines through the chunked map_and_process, as the product does when the device path declines a file: a plain
    file's handle, a gzip file's inflating handle, a BAM's SAM rendering line by line."""
    cov = tmp_path / (tag + ".chunked.tsv")
    args = sc.make_args(str(path), str(dbinfo), str(tmp_path / (tag + ".c.cami")), {"coverage": str(cov)})
    acc2info, taxid2info = mp.get_acc2info(args)

    def stream():
        if path.name.endswith(".bam"):
            return None, mp.bam.sam_lines(str(path))
        fh = gzip.open(path, "rb") if path.name.endswith(".gz") else open(path, "rb")
        return fh, fh
    cv.write_coverage(str(cov))
    fh, lines = stream()
    t2a, mm, _ = mp.map_and_process(args, lines, acc2info, taxid2info, _coverage=str(path))
    if fh:
        fh.close()
    fh, lines = stream()
    t2a0, mm0, _ = mp.map_and_process(args, lines, acc2info, taxid2info)
    if fh:
        fh.close()
    assert t2a == t2a0 and mm == mm0, tag
    return cov.read_bytes()


def _every_mode(d, stem, lines, dbinfo, tmp_path, monkeypatch):
    """The issue's matrix for one file: as .sam, .sam.gz and .bam — default, many pieces, whole text, the chunked path, with
    --read_assignments, and (the lines in coordinate order) with --collate always.  In every case the coverage file is the
    definition's bytes and the profile is the one the run without the flag writes."""
    from metalign_amd import assignments as asg
    want = _definition_bytes(lines, dbinfo)
    acc2info, _ = mp.get_acc2info(sc.make_args("-", dbinfo, "-", {}))
    want_rows = (asg.HEADER + "".join(asg.format_row(r) for r in asg.read_assignments(lines, acc2info, 0.5))).encode()
    forms = _three_forms(d, stem, lines)
    kw = dict(input_type="sam", db="unused.fna")

    def both(path, tag, **more):
        cami, cov = _run(path, dbinfo, tmp_path, tag, **kw, **more)
        cami0, none = _run(path, dbinfo, tmp_path, tag + "_0", cov=False, **kw, **more)
        assert none is None and cami == cami0, (tag, path.name)
        return cov

    plain = {}
    for path in forms:
        assert both(path, "default") == want, path.name
        plain[path] = (tmp_path / "default_0.cami").read_text()
        rows = tmp_path / (path.name + ".reads.tsv")
        assert both(path, "rows", read_assignments=str(rows)) == want and rows.read_bytes() == want_rows, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))  # many pieces
        for path in forms:
            assert both(path, "pieces") == want, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_NO_STREAM", "1")  # the whole text in one tokeniser call (a compressed file is streamed all the same)
        for path in forms:
            if path.name.endswith(".gz"):
                # without the flag the whole-text call is handed the compressed bytes (it has no inflater in front of it, a
                # limitation this flag leaves alone): the profile is held to the default mode's run without the flag instead
                cami, cov = _run(path, dbinfo, tmp_path, "whole", **kw)
                assert cov == want and cami == plain[path], path.name
            else:
                assert both(path, "whole") == want, path.name
    with monkeypatch.context() as m:
        m.setattr(mp, "_CHUNK_BYTES", 40000)  # many chunks
        for path in forms:
            assert _chunked(path, dbinfo, tmp_path, path.name) == want, path.name
    shuffled = collate_cases.coordinate_shuffle("".join(lines))  # (POS drawn anew, the lines in coordinate order)
    grouped = list(collate.collated_lines(shuffled))             # the same lines, every read's together again: the unshuffled file
    want_s = _definition_bytes(shuffled, dbinfo)
    assert want_s == _definition_bytes(grouped, dbinfo)
    (tmp_path / "grouped.sam").write_text("".join(grouped))
    assert _run(tmp_path / "grouped.sam", dbinfo, tmp_path, "grouped")[1] == want_s
    for path in _three_forms(tmp_path, stem + "_shuffled", shuffled):
        assert both(path, "col", collate="always") == want_s, path.name
    return forms, want, want_s


@pytest.mark.parametrize("name", ["cascade_break", "paired_mix", "multimap_split", "species_and_virus"])
def test_map_main_hand_cases_in_every_form_and_mode(hip, tmp_path, monkeypatch, name):
    cdir = os.path.join(sc.GOLDEN, "cases")
    dbinfo = os.path.join(cdir, "dbinfo.txt")
    lines = _dressed(os.path.join(cdir, name + ".sam"), dbinfo, 31)
    forms, want, want_s = _every_mode(tmp_path, name, lines, dbinfo, tmp_path, monkeypatch)
    assert want.count(b"\nS\t") >= 1 and want.count(b"\nG\t") >= 1


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("coverage_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = _dressed(sam, dbinfo, 32)
    forms = _three_forms(d, "b", lines)
    return d, forms, dbinfo, lines, _definition_bytes(lines, dbinfo)


def test_map_main_bulk_in_every_form_and_mode(hip, bulk, tmp_path, monkeypatch):
    d, forms, dbinfo, lines, want = bulk
    assert want.count(b"\n") > 20 and int(want.rsplit(b"\t", 1)[1]) > 50  # (rows, and unplaced alignments)
    _, got_want, want_s = _every_mode(tmp_path, "bulk", lines, dbinfo, tmp_path, monkeypatch)
    assert got_want == want and want_s.count(b"\n") > 20
    cami0, _ = _run(forms[0], dbinfo, tmp_path, "plain", cov=False)  # (one profile, whatever the form)
    for path in forms[1:]:
        assert _run(path, dbinfo, tmp_path, "form", input_type="sam", db="unused.fna")[0] == cami0.replace(str(forms[0]), str(path))


def test_two_input_files_give_two_blocks(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, want = bulk
    out, cov = tmp_path / "two.cami", tmp_path / "two.tsv"
    args = sc.make_args(str(forms[0]), str(dbinfo), str(out), {"input_type": "AUTO", "coverage": str(cov)})
    args.infiles = [str(forms[0]), str(forms[2])]
    mp.map_main(args)
    assert cov.read_bytes() == (_definition_bytes(lines, dbinfo, source=str(forms[0]))
                                + _definition_bytes(lines, dbinfo, source=str(forms[2]), header=False))


def test_a_chunk_the_host_tokeniser_takes_brings_its_places(hip, bulk, tmp_path, monkeypatch):
    """FLAG 1_6 is 16 to Python's int() and no number to the device parser: that chunk goes through the host tokeniser, and its
    places through coverage.placement."""
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
    cami, cov = _run(sam, dbinfo, tmp_path, "odd")
    assert cov == want
    assert cami == _run(sam, dbinfo, tmp_path, "odd0", cov=False)[0]
