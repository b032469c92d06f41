"""-m gpu: coordinate-sorted SAM / BAM files collated by read on the device (metalign_amd/csrc/mg_collate.hip).

The definition is metalign_amd/collate.py: every expected value comes from collated_lines of the file at hand — the profile of a
collated file is the reference's profile OF THE COLLATED TEXT (its loop depends on the order of the reads), never that of the
name-grouped file the input was shuffled from."""
import functools
import random

import numpy as np
import pytest

import bamgen
import collate_cases as cc
import indep_sketch
import stage_c_checks as sc
from metalign_amd import _hip, collate
from metalign_amd import map_and_profile as mp
from test_bam_core_host import bad_lines, edge_lines

pytestmark = pytest.mark.gpu

_DEFAULT_INFLATE = dict(chunk_bytes=32 << 10, stage_bytes=-1, ratio=10, on=1, lane_jobs=1 << 40)
FLAGS = np.array([0, 16, 256, 2048, 99, 147, 355, 403, 65, 129, 193], dtype=np.uint32)
SMALL, BIG = (300, 100), (20000, 4000)


@pytest.fixture()
def inflate(hip):
    yield hip.inflate_config
    hip.inflate_config(**_DEFAULT_INFLATE)


@functools.lru_cache(maxsize=None)
def _shuffled(size):
    """-> (dbinfo text, accs, acc_index, the name-grouped text, its coordinate shuffle as lines, the records of the collated shuffle)"""
    dbinfo, accs, acc_index, text = cc.case(*size)
    lines = cc.coordinate_shuffle(text)
    want = mp.tokenise_sam(collate.collated_lines(lines), acc_index)
    want.setflags(write=False)
    return dbinfo, accs, acc_index, text, lines, want


def _index(hip, acc_index):
    return hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])


def _line(q, flag, acc):
    return "%s\t%d\t%s\t7\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\n" % (q, flag, acc)


# ---- 1. keys ----
def test_device_keys_equal_the_host_cores_for_sam_and_bam(hip):
    _, accs, acc_index, _, _, _ = _shuffled(SMALL)
    names = [n.decode() for n in cc.KEY_NAMES]
    lines = []
    for i, n in enumerate(names):
        lines.append(_line(n, (0, 16, 256, 99)[i & 3], accs[i % len(accs)]))
        if i % 3 == 0:
            lines.append(_line("unmapped%d" % i, 4, "*"))  # (not retained: no key)
    want = np.array([indep_sketch.murmur3_x64_128(n.encode(), cc.SEED) for n in names], dtype=np.uint64)
    idx = _index(hip, acc_index)
    text = np.frombuffer("".join(lines).encode(), dtype=np.uint8)
    data, hdr, refs = bamgen.encode(lines)
    stream = np.frombuffer(data[hdr:], dtype=np.uint8)
    d_t, d_b = hip.array(text), hip.array(stream)
    try:
        a = hip.sam_tokenize_keyed_dev(d_t.ptr, text.size, idx)
        b, used = hip.bam_tokenize_dev(d_b.ptr, stream.size, np.array([acc_index.get(n, -1) for n in refs], dtype=np.int32), idx, keyed=True)
        try:
            assert used == stream.size and a.count == b.count == len(names)
            assert np.array_equal(a.keys(), want) and np.array_equal(b.keys(), want)
            assert np.array_equal(a.download(), b.download())
            plain = hip.sam_tokenize_dev_batch(d_t.ptr, text.size, idx)
            with pytest.raises(_hip.HipError):  # a batch without keys says so
                plain.keys()
            assert np.array_equal(plain.download(), a.download())
            plain.free()
        finally:
            a.free()
            b.free()
    finally:
        d_t.free()
        d_b.free()
        idx.free()


@pytest.mark.parametrize("how", ["host inflater", "device inflater"])
def test_keys_of_a_file_tokenised_in_pieces_equal_one_call(hip, tmp_path, inflate, knobs, how):
    """The collated stream calls, stopped before the collation (knob collate_defer): records and keys of the pieces, appended, equal
    one keyed call on the whole text; collating that batch then gives the definition's records."""
    _, accs, acc_index, _, _, _ = _shuffled(SMALL)
    _, _, _, text = cc.case(3000, 800)
    lines = cc.coordinate_shuffle(text)
    body = "".join(lines)
    want = mp.tokenise_sam(collate.collated_lines(lines), acc_index)
    inflate(on=0 if how.startswith("host") else 1)
    if not how.startswith("host"):
        inflate(chunk_bytes=4 << 10, stage_bytes=64 << 10)
    idx = _index(hip, acc_index)
    raw = np.frombuffer(body.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    try:
        one = hip.sam_tokenize_keyed_dev(d_t.ptr, raw.size, idx)
        keys, recs = one.keys(), one.download()
        one.free()
        assert len(keys) == len(want) > 3000 and len(body) > 8 << 16
        files = []
        p = tmp_path / "x.sam"
        p.write_text(body)
        files.append((p, False))
        for block in (1024, 5000):
            p = tmp_path / ("x_%d.sam.gz" % block)
            p.write_bytes(bamgen.bgzf_text(body, block=block))
            files.append((p, False))
            p = tmp_path / ("x_%d.bam" % block)
            p.write_bytes(bamgen.sam_to_bam(body, block=block))
            files.append((p, True))
        knobs("collate_defer", 1)
        for p, is_bam in files:
            b = (hip.bam_stream_file(str(p), idx, chunk_bytes=1 << 16, collate=True) if is_bam
                 else hip.sam_stream_file(str(p), idx, chunk_bytes=1 << 16, collate=True))
            try:
                assert np.array_equal(b.keys(), keys), p.name
                assert np.array_equal(b.download(), recs), p.name
                perm = b.collate(want_perm=True)
                got = b.download()
                assert np.array_equal(got, want), p.name
                assert np.array_equal(got["flag_len"], recs["flag_len"][perm.astype(np.int64)])
                with pytest.raises(_hip.HipError):  # collated once: the keys are gone
                    b.collate()
            finally:
                b.free()
    finally:
        d_t.free()
        idx.free()


# ---- 2. the order, on hand-made keys ----
def _want_perm(keys, flags):
    """numpy lexsort of the definition: the group id is the index of the key's first appearance."""
    n = len(flags)
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    both = np.ascontiguousarray(keys).view([("lo", "<u8"), ("hi", "<u8")]).reshape(n)
    _, first, inverse = np.unique(both, return_index=True, return_inverse=True)
    gid = first[inverse.reshape(n)]
    mate2 = ((flags & 1) != 0) & ((flags & 128) != 0) & ((flags & 64) == 0)
    notprimary = (flags & 0x900) != 0
    return np.lexsort((np.arange(n), notprimary, mate2, gid)).astype(np.uint64)


def _key_patterns(n, rng):
    wide = lambda size: rng.integers(0, 1 << 64, size=size, dtype=np.uint64)  # noqa: E731
    out = {}
    out["all equal"] = np.tile(np.array([[0xF123456789ABCDEF, 7]], dtype=np.uint64), (n, 1))
    out["all distinct"] = np.stack([wide(n), wide(n)], axis=1)
    out["all distinct"][:, 0] ^= np.arange(n, dtype=np.uint64)  # (distinct whatever the draw: hi is drawn once more below)
    out["all distinct"][:, 1] = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    m = (n + 1) // 2
    half = np.stack([wide(m), wide(m)], axis=1)
    out["every name twice, far apart"] = np.concatenate([half, half])[:n]
    few = max(1, n // 3)
    out["runs share hi, not lo"] = np.stack([wide(few)[rng.integers(0, few, size=n)], np.full(n, 1 << 63, dtype=np.uint64)], axis=1)
    out["runs share lo, not hi"] = np.stack([np.full(n, 3, dtype=np.uint64), wide(few)[rng.integers(0, few, size=n)]], axis=1)
    alt = np.stack([wide(few)[rng.integers(0, few, size=n)], (np.arange(n, dtype=np.uint64) & np.uint64(1)) << np.uint64(63)], axis=1)
    out["a name's two neighbours differ in one half only"] = alt
    last = np.stack([wide(few)[rng.integers(0, few, size=n)] | np.uint64(1), wide(few)[rng.integers(0, few, size=n)]], axis=1)
    last[n - 1] = (0, 0)  # the smallest key: first after the key sort, the LAST group of the file
    out["the smallest key last in the file"] = last
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4097, 70000])
def test_order_on_raw_keys_equals_the_definition(hip, n):
    rng = np.random.default_rng(1000 + n)
    if n == 0:
        assert len(hip.collate_order(np.zeros((0, 2), np.uint64), np.zeros(0, _hip.REC_DTYPE))) == 0
        return
    for name, keys in _key_patterns(n, rng).items():
        flags = FLAGS[rng.integers(0, len(FLAGS), size=n)]
        recs = np.zeros(n, dtype=_hip.REC_DTYPE)
        recs["ref_new"] = rng.integers(0, 1 << 31, size=n, dtype=np.uint32) | np.uint32(_hip.NEW_BIT)
        recs["flag_len"] = flags | (rng.integers(0, 300, size=n, dtype=np.uint32) << np.uint32(_hip.LEN_SHIFT))
        got = hip.collate_order(keys, recs)
        want = _want_perm(keys, flags)
        assert np.array_equal(got, want), (n, name, int(np.argmax(got != want)))


# ---- 3. records ----
@pytest.mark.parametrize("how", ["host inflater", "device inflater"])
@pytest.mark.parametrize("size", [SMALL, BIG], ids=["300+100", "20000+4000"])
def test_collated_records_equal_the_definition(hip, tmp_path, inflate, size, how):
    _, accs, acc_index, _, lines, want = _shuffled(size)
    body = "".join(lines)
    inflate(on=0 if how.startswith("host") else 1)
    if not how.startswith("host"):
        inflate(chunk_bytes=4 << 10, stage_bytes=64 << 10)
    # (the shuffle scattered the reads: what "never" sees is something else)
    assert not np.array_equal(mp.tokenise_sam(lines, acc_index), want)
    idx = _index(hip, acc_index)
    try:
        sam = tmp_path / "x.sam"
        sam.write_text(body)
        cases = [("sam", sam, False, 1 << 16), ("sam, one piece", sam, False, 0)]
        for block in (1024, 5000):
            gz, bm = tmp_path / ("x_%d.sam.gz" % block), tmp_path / ("x_%d.bam" % block)
            gz.write_bytes(bamgen.bgzf_text(body, block=block))
            bm.write_bytes(bamgen.sam_to_bam(body, block=block))
            cases += [("sam.gz %d" % block, gz, False, 1 << 16), ("bam %d" % block, bm, True, 1 << 16)]
        for name, p, is_bam, chunk in cases:
            b = (hip.bam_stream_file(str(p), idx, chunk_bytes=chunk, collate=True) if is_bam
                 else hip.sam_stream_file(str(p), idx, chunk_bytes=chunk, collate=True))
            try:
                assert b.count == len(want)
                assert np.array_equal(b.download(), want), name
            finally:
                b.free()
    finally:
        idx.free()


def test_empty_and_single_record_files(hip, tmp_path):
    _, accs, acc_index, _, _, _ = _shuffled(SMALL)
    idx = _index(hip, acc_index)
    try:
        for name, lines in (("none", ["@HD\tVN:1.6\tSO:coordinate\n", _line("u", 4, "*")]), ("one", [_line("r", 16, accs[0])]), ("nothing", [])):
            p = tmp_path / (name + ".sam")
            p.write_text("".join(lines))
            b = hip.sam_stream_file(str(p), idx, collate=True)
            try:
                assert np.array_equal(b.download(), mp.tokenise_sam(collate.collated_lines(lines), acc_index))
            finally:
                b.free()
    finally:
        idx.free()


# ---- 4. map_main ----
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("collate_files")
    dbinfo_text, accs, acc_index, text, lines, _ = _shuffled(BIG)
    (d / "db_info.txt").write_text(dbinfo_text)
    (d / "shuffled.sam").write_text("".join(lines))
    (d / "shuffled.bam").write_bytes(bamgen.sam_to_bam("".join(lines), block=20000))
    (d / "collated.sam").write_text("".join(collate.collated_lines(lines)))
    (d / "grouped.sam").write_text(text)
    unsorted = cc.coordinate_shuffle(text, so="unsorted")
    (d / "says_unsorted.sam").write_text("".join(unsorted))
    (d / "says_unsorted.bam").write_bytes(bamgen.sam_to_bam("".join(unsorted), block=20000))
    return d


def _run(files, tmp_path, name, **extra):
    out = tmp_path / (name.replace(".", "_") + "_" + "_".join("%s" % v for v in extra.values()) + ".tsv")
    mp.map_main(sc.make_args(str(files / name), str(files / "db_info.txt"), str(out), dict({"input_type": "AUTO", "sampleID": "s"}, **extra)))
    return out.read_text()


def _rows(text):
    return [ln.split("\t") for ln in text.splitlines() if ln and ln[0] != "@"]


def test_map_main_always_gives_the_profile_of_the_collated_text(hip, files, tmp_path, monkeypatch):
    monkeypatch.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))
    want = _run(files, tmp_path, "collated.sam")
    assert want.count("\n") > 20
    sam = _run(files, tmp_path, "shuffled.sam", collate="always")
    bm = _run(files, tmp_path, "shuffled.bam", collate="always")
    assert sam == want and bm == want
    # the discriminating condition: profiled as it is, the shuffled file gives something else (nearly every read "unmapped")
    assert _run(files, tmp_path, "shuffled.sam", collate="never") != want
    assert _run(files, tmp_path, "shuffled.sam") != want  # (no option at all: never)
    for name in ("shuffled.sam", "shuffled.bam"):
        dm = _rows(_run(files, tmp_path, name, collate="always", device_multimap=True))
        assert [r[0] for r in dm] == [r[0] for r in _rows(want)]
        assert all(abs(float(x[4]) - float(y[4])) <= 1e-6 for x, y in zip(dm, _rows(want)))


def test_map_main_auto_follows_the_header(hip, files, tmp_path):
    always = _run(files, tmp_path, "shuffled.sam", collate="always")
    for name in ("shuffled.sam", "shuffled.bam"):
        assert _run(files, tmp_path, name, collate="auto") == always
    for name in ("says_unsorted.sam", "says_unsorted.bam"):
        never = _run(files, tmp_path, name, collate="never")
        assert _run(files, tmp_path, name, collate="auto") == never != always


def test_map_main_always_on_name_grouped_output_changes_nothing(hip, files, tmp_path):
    assert _run(files, tmp_path, "grouped.sam", collate="always") == _run(files, tmp_path, "grouped.sam", collate="never")


def test_the_warning_points_to_the_option_unless_collating(hip, files, tmp_path, capsys):
    _run(files, tmp_path, "shuffled.bam", collate="never")
    err = capsys.readouterr().err
    assert "sorted by coordinate" in err and "--collate" in err
    _run(files, tmp_path, "shuffled.bam", collate="always")
    assert "sorted by coordinate" not in capsys.readouterr().err


# ---- 5. fallback ----
def test_a_record_the_device_does_not_decide_goes_through_the_host_definition(hip, tmp_path):
    dbinfo_text, accs, acc_index, _, lines, _ = _shuffled(SMALL)
    (tmp_path / "db_info.txt").write_text(dbinfo_text)
    floating = edge_lines(accs)[-1]
    assert "Xf:f:" in floating
    every = lines + [floating]
    bm = tmp_path / "float.bam"
    bm.write_bytes(bamgen.sam_to_bam("".join(every), block=3000))
    idx = _index(hip, acc_index)
    try:
        with pytest.raises(_hip.SamParseError) as e:  # (the device hands the file back: kind 6)
            hip.bam_stream_file(str(bm), idx, collate=True)
        assert e.value.kind == 6
    finally:
        idx.free()
    (tmp_path / "want.sam").write_text("".join(collate.collated_lines(every)))
    want = _run(tmp_path, tmp_path, "want.sam")
    assert _run(tmp_path, tmp_path, "float.bam", collate="always") == want and want.count("\n") > 10
    assert _run(tmp_path, tmp_path, "float.bam", collate="never") != want


def test_a_line_the_reference_cannot_parse_raises_what_the_definition_raises(hip, tmp_path):
    dbinfo_text, accs, acc_index, _, lines, _ = _shuffled(SMALL)
    (tmp_path / "db_info.txt").write_text(dbinfo_text)
    for i, (line, exc) in enumerate(bad_lines(accs)[1:4]):  # an unknown reference, an '=' operation, a CIGAR of no length
        every = lines[:200] + [line] + lines[200:]
        with pytest.raises(exc):
            mp.tokenise_sam(collate.collated_lines(every), acc_index)
        (tmp_path / ("bad%d.sam" % i)).write_text("".join(every))
        (tmp_path / ("bad%d.bam" % i)).write_bytes(bamgen.sam_to_bam("".join(every), block=3000))
        for name in ("bad%d.sam" % i, "bad%d.bam" % i):
            with pytest.raises(exc):
                _run(tmp_path, tmp_path, name, collate="always")
