"""-m gpu: --read_assignments on the device — stage C's verdict words (mg_profile_commit_assign_dev), the named tokenisers and the
command line.  The expectation is always metalign_amd/assignments.py (read_assignments) of the file at hand."""
import functools
import gzip
import random

import numpy as np
import pytest

import bamgen
import samgen
import stage_c_checks as sc
from metalign_amd import _hip
from metalign_amd import assignments as asg
from metalign_amd import collate
from metalign_amd import map_and_profile as mp
from metalign_amd.distributed import compose_incoming

pytestmark = pytest.mark.gpu

TILE, HALO = 2048, 64
PCT = 0.5


@functools.lru_cache(maxsize=None)
def _db():
    """-> (db_info text, accessions, acc2info, taxid2info, acc_index, taxids, ref2tax)"""
    text, accs, _ = samgen.make_dbinfo(seed=11, n_species=40)
    acc2info, taxid2info = {}, {}
    for row in text.splitlines()[1:]:
        acc, acclen, taxid, namelin, taxlin = row.split("\t")
        rank = mp.get_taxid_rank(taxlin)
        if rank == "strain" and acc != "Unmapped":
            taxid, taxlin = taxid + ".1", taxlin + ".1"
        acc2info[acc] = [int(acclen), taxid, namelin, taxlin]
        taxid2info.setdefault(taxid, [0, rank, namelin, taxlin])[0] += int(acclen)
    acc_index, taxids, ref2tax = mp.dense_tables(acc2info, taxid2info)
    return text, accs, acc2info, taxid2info, acc_index, taxids, ref2tax


def _retained(lines):
    return [ln for ln in lines if asg._fields_of(ln) is not None]


def _with_more_failing_lines(lines, seed, share=0.3):
    """Every retained line's CIGAR replaced, with probability `share`, by one that fails pct_id: runs of Ambiguous reads, each
    taking the next read's first line, long enough to cross tile edges."""
    rng = random.Random(seed)
    out = []
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        if rng.random() < share:
            n = 40 if f[9] == "*" else len(f[9])
            f[5] = samgen._cigar_bad(rng, n)
        out.append("\t".join(f) + "\n")
    return out


@functools.lru_cache(maxsize=None)
def _stream(kind, nrecs):
    """A seeded SAM stream cut to exactly nrecs retained lines."""
    _, accs, _, _, _, _, _ = _db()
    taxid_of = [_db()[2][a][1] for a in accs]
    gen = samgen.make_sam_single if kind == "single" else samgen.make_sam_paired
    text = gen(77 + nrecs, nrecs, accs, taxid_of)  # (a read or a pair gives at least ~1 retained line: more than enough)
    lines = _with_more_failing_lines(_retained(text.splitlines(True)), nrecs)
    assert len(lines) >= nrecs
    return tuple(lines[:nrecs])


class _Held:
    def __init__(self):
        self.items = []

    def __call__(self, x):
        self.items.append(x)
        return x

    def free(self):
        for x in reversed(self.items):
            x.free()


def _commit(hip, recs, ref2tax, ntax, assign, bounds=None):
    """Stage C through the C ABI over `recs`, as one shard or cut at `bounds`: -> (accumulators, CSR (offsets, taxa, hitlen, read),
    verdict words or None).  Shards: lookahead record, composed incoming state, running group_base; the multimapped rows of the
    later shards' words are moved up by the multimapped reads in front of them (a word holds the row in its OWN shard's CSR)."""
    held = _Held()
    try:
        T = max(ntax, 1)
        bounds = [0, len(recs)] if bounds is None else bounds
        d_r2t = held(hip.array(ref2tax))
        d_acc = held(hip.empty(3 * T + 2, np.uint64))
        base = d_acc.ptr
        hip._chk(hip.lib.mg_profile_acc_reset(_hip._vp(base), _hip._vp(base + 8 * T), _hip._vp(base + 16 * T), _hip._vp(base + 24 * T),
                                              _hip.ctypes.c_uint32(ntax)))
        shards = []
        for a, b in zip(bounds, bounds[1:]):
            look = b < len(recs)
            part = recs[a:b + (1 if look else 0)]
            d = held(hip.array(part if len(part) else np.zeros(1, _hip.REC_DTYPE)))
            shards.append(held(hip.profile_begin_dev(d.ptr, b - a, look, d_r2t.ptr, len(ref2tax), ntax, PCT)))
        maps = [s.state_map() for s in shards]
        groups = [s.ngroups for s in shards]
        words, csr, mm_before = [], [], 0
        for i, s in enumerate(shards):
            args = (compose_incoming(maps, i), i == 0, sum(groups[:i]), base, base + 8 * T, base + 16 * T, base + 24 * T)
            if assign:
                d_w = held(hip.array(np.full(max(2 * groups[i], 2) + 2, 0xABABABABABABABAB, dtype=np.uint64)))
                s.commit_assign(*args, d_w.ptr)
                w = d_w.download()
                assert np.all(w[2 * groups[i]:] == 0xABABABABABABABAB), "words written past the shard's reads"
                w = w[:2 * groups[i]].copy()
                multi = (w[0::2] & 3) == 2
                w[1::2][multi] += np.uint64(mm_before)
                words.append(w)
            else:
                s.commit(*args)
            csr.append(s.multimapped() if bounds[i + 1] > bounds[i] else (np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)))
            mm_before += len(csr[-1][2])
        acc = d_acc.download()
        off, at = [np.zeros(1, np.uint64)], 0
        for o, t, _, _ in csr:
            off.append(o[1:] + np.uint64(at))
            at += len(t)
        merged = (np.concatenate(off), np.concatenate([c[1] for c in csr]), np.concatenate([c[2] for c in csr]),
                  np.concatenate([c[3] for c in csr]))
        return acc, merged, (np.concatenate(words) if assign else None)
    finally:
        held.free()


def _check_words(hip, lines, bounds_of=None):
    """The device's words over the records of `lines` against the definition; the sums and the CSR against the plain commit."""
    _, _, acc2info, _, acc_index, taxids, ref2tax = _db()
    want = list(asg.read_assignments(lines, acc2info, PCT))
    recs = mp.tokenise_sam(lines, acc_index)
    acc0, csr0, _ = _commit(hip, recs, ref2tax, len(taxids), assign=False)
    acc1, csr1, words = _commit(hip, recs, ref2tax, len(taxids), assign=True)
    assert np.array_equal(acc0, acc1), "the variant changed count / bases / first_seen / scalars"
    assert all(np.array_equal(x, y) for x, y in zip(csr0, csr1)), "the variant changed the multimapped CSR"
    names = mp._pack_names([r[0] for r in want])
    got = list(asg.rows_from_words(words, names[0], names[1], taxids, csr1[0], csr1[1], csr1[2]))
    assert len(got) == len(want) == int(acc1[3 * max(len(taxids), 1)])
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]
    if bounds_of is not None:
        bounds = bounds_of(recs)
        acc2, csr2, words2 = _commit(hip, recs, ref2tax, len(taxids), assign=True, bounds=bounds)
        assert np.array_equal(acc2, acc1) and all(np.array_equal(x, y) for x, y in zip(csr2, csr1))
        assert np.array_equal(words2, words), "the shards' words, one behind the other, differ from the single shard's"
    return want


@pytest.mark.parametrize("kind", ["single", "paired"])
@pytest.mark.parametrize("nrecs", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_verdict_words_equal_the_definition(hip, kind, nrecs):
    want = _check_words(hip, list(_stream(kind, nrecs)))
    assert want[-1][1] == "N"
    if nrecs > TILE:
        cls = "".join(r[1] for r in want)
        assert "AAA" in cls and "U" in cls and "M" in cls  # (chains of dropped first lines, and the other two classes)


def _hand(q, flag, acc, seq="ACGTACGTAC", cigar=None):
    return samgen._line(q, flag, acc, cigar or ("%dM" % (10 if seq == "*" else len(seq))), seq, 0)


def _filler(accs, n, start=0):
    """n single-line reads f<start> .. (each loses or keeps its line as the chain before it decides)."""
    return [_hand("f%d" % (start + i), 0 if i % 3 else 16, accs[(start + i) % len(accs)], cigar="2M8S" if i % 7 == 3 else None)
            for i in range(n)]


def test_long_reads_beyond_the_halo_and_across_tiles(hip):
    accs = _db()[1]
    lines = _filler(accs, 100)
    lines += [_hand("halo65", 0, accs[1])] + [_hand("halo65", 256, accs[(2 + i) % 9], seq="*") for i in range(HALO)]  # 65 lines
    lines += _filler(accs, 1500, 100)
    lines += [_hand("long2100", 0, accs[3])] + [_hand("long2100", 256, accs[(i * 5) % 11], seq="*") for i in range(2099)]  # spans tiles
    lines += _filler(accs, 50, 1600)
    lines += [_hand("pairlong", 99, accs[4])] + [_hand("pairlong", 355, accs[4 + i % 3], seq="*") for i in range(70)]
    lines += [_hand("pairlong", 147, accs[4])] + [_hand("pairlong", 403, accs[4 + i % 3], seq="*") for i in range(70)]  # both mates mapped
    lines += [_hand("tail", 99, accs[5]), _hand("tail", 147, accs[5]), _hand("end", 0, accs[0])]
    want = _check_words(hip, lines)
    by_name = {r[0]: r for r in want}
    assert by_name["halo65"][1] == "M" and by_name["long2100"][1] == "M" and len(by_name["long2100"][2]) >= 2099
    assert by_name["pairlong"][1] in "MU"


def test_a_read_closing_on_a_tiles_last_record_and_the_last_read_across_the_final_edge(hip):
    accs = _db()[1]
    lines = _filler(accs, TILE - 3)
    lines += [_hand("closes", 0, accs[1]), _hand("closes", 256, accs[2], seq="*"), _hand("closes", 256, accs[7], seq="*")]
    assert len(lines) == TILE  # ("closes" ends on record TILE - 1; the line that closes it is the next tile's first)
    lines += _filler(accs, TILE - 2, 5000)
    lines += [_hand("last", 0, accs[3])] + [_hand("last", 256, accs[4], seq="*") for _ in range(6)]  # records 2 TILE - 2 .. 2 TILE + 4
    want = _check_words(hip, lines)
    assert want[-1] == ("last", "N", [], -1)
    assert {r[0]: r for r in want}["closes"][1] == "M"


def test_three_shards_give_the_single_shards_words(hip):
    def cuts(recs):
        new = np.nonzero(recs["ref_new"] >> 31)[0]
        a = int(new[np.searchsorted(new, len(recs) // 3)])        # read boundaries, away from the tile edges
        b = int(new[np.searchsorted(new, 2 * len(recs) // 3 + 17)])
        assert 0 < a < b < len(recs) and a % TILE and b % TILE
        return [0, a, b, len(recs)]
    for kind in ("single", "paired"):
        _check_words(hip, list(_stream(kind, 3 * TILE + 5)), bounds_of=cuts)


# ---- names ---------------------------------------------------------------------------------------------------------------
def _name_lines():
    accs = _db()[1]
    rng = random.Random(5)
    lens = [1, 2, 63, 64, 65, 254]
    names = []
    for rep in range(180):  # shared prefixes: the same stem cut to every length, then the stem changes in its LAST position
        stem = ("stem%02d_" % (rep // 6)) + "x" * 254
        for n in lens:
            names.append((stem[:n - 1] + "abcdefghijklmnopqrstuvwxyz0123456789"[rep % 36])[:n] if n > 1 else "abcdefghijklmnopqrstuvwxyz0123456789"[rep % 36])
    lines = ["@HD\tVN:1.6\tSO:unsorted\n"]
    for i, q in enumerate(names):
        lines.append(_hand(q, 0, accs[i % len(accs)]))
        for _ in range(rng.randrange(0, 4)):
            lines.append(_hand(q, 256, accs[rng.randrange(len(accs))], seq="*"))
        if i % 5 == 0:
            lines.append(_hand("unmapped%d" % i, 4, "*", cigar="*"))
    return lines


def _index(hip):
    acc_index = _db()[4]
    return hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])


def _want_names(lines):
    acc2info = _db()[2]
    return mp._pack_names([r[0] for r in asg.read_assignments(lines, acc2info, PCT)])


def _names_of(batch):
    try:
        return batch.names(), batch.download()
    finally:
        batch.free()


def test_names_are_the_same_whole_streamed_bgzf_and_bam(hip, tmp_path, monkeypatch):
    lines = _name_lines()
    text = "".join(lines)
    want_blob, want_off = _want_names(lines)
    assert len(want_off) - 1 == 1080 and len(text) > 5 * (1 << 16) and {int(x) for x in np.diff(want_off)} == {1, 2, 63, 64, 65, 254}
    want_recs = mp.tokenise_sam(lines, _db()[4])
    idx = _index(hip)
    (tmp_path / "n.sam").write_text(text)
    # (stored BGZF members: the compressed files are as long as the text, so they too come in several pieces)
    (tmp_path / "n.sam.gz").write_bytes(bamgen.bgzf(text.encode(), block=4000, level=0))
    (tmp_path / "n.bam").write_bytes(bamgen.sam_to_bam(text, block=4000, level=0))
    got = {}
    raw = np.frombuffer(text.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    try:
        got["whole text"] = _names_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, named=True))
        recs, last, nm = hip.sam_tokenize(text.encode(), idx, named=True)
        got["host text"] = (nm, recs)
        # the smallest piece the pipeline takes is 64 KB: five or more pieces of this text, the reads with secondaries span their edges
        got["streamed"] = _names_of(hip.sam_stream_file(str(tmp_path / "n.sam"), idx, chunk_bytes=1 << 12, named=True))
        got["streamed, one piece"] = _names_of(hip.sam_stream_file(str(tmp_path / "n.sam"), idx, named=True))
        got["bgzf"] = _names_of(hip.sam_stream_file(str(tmp_path / "n.sam.gz"), idx, chunk_bytes=1 << 12, named=True))
        got["bam"] = _names_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, chunk_bytes=1 << 12, named=True))
        got["bam, one piece"] = _names_of(hip.bam_stream_file(str(tmp_path / "n.bam"), idx, named=True))
        for how, ((blob, off), recs) in got.items():
            assert np.array_equal(off, want_off), how
            assert blob == want_blob, how
            assert np.array_equal(recs, want_recs), how
        # a batch without names says so; a named batch is not collated
        plain = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx)
        with pytest.raises(_hip.HipError) as e:
            plain.names()
        assert e.value.code == _hip.ERR_STATE
        plain.free()
        named = hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, named=True)
        with pytest.raises(_hip.HipError) as e:
            named.collate()
        assert e.value.code == _hip.ERR_STATE
        named.free()
        empty = hip.sam_tokenize_dev_batch(d_t.ptr, 0, idx, named=True)
        (blob, off), recs = _names_of(empty)
        assert blob == b"" and list(off) == [0] and len(recs) == 0
    finally:
        d_t.free()
        idx.free()


def test_names_of_a_paf_replay(hip):
    from test_gpu_paf import _sam_stream, _to_paf
    _, accs, acc2info, _, acc_index, _, _ = _db()
    sam = _sam_stream(3, 400, accs, [acc2info[a][1] for a in accs])
    paf = "".join(_to_paf(ln) for ln in sam)
    idx = _index(hip)
    raw = np.frombuffer(paf.encode(), dtype=np.uint8)
    d_t = hip.array(raw)
    try:
        (blob, off), recs = _names_of(hip.sam_tokenize_dev_batch(d_t.ptr, raw.size, idx, paf=True, named=True))
        want_blob, want_off = _want_names(sam)
        assert blob == want_blob and np.array_equal(off, want_off)
        assert np.array_equal(recs, mp.tokenise_paf(paf.splitlines(True), acc_index))
    finally:
        d_t.free()
        idx.free()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _definition_bytes(lines, dbinfo_path, pct_id=0.5):
    args = sc.make_args("-", dbinfo_path, "-", {})
    acc2info, _ = mp.get_acc2info(args)
    return (asg.HEADER + "".join(asg.format_row(r) for r in asg.read_assignments(lines, acc2info, pct_id))).encode()


def _run(sam, dbinfo, tmp_path, tag, **extra):
    out, rows = tmp_path / (tag + ".cami"), tmp_path / (tag + ".reads.tsv")
    ov = dict({"input_type": "AUTO", "sampleID": "s"}, **extra)
    if ov.pop("rows", True):
        ov["read_assignments"] = str(rows)
    mp.map_main(sc.make_args(str(sam), str(dbinfo), str(out), ov))
    return out.read_text(), (rows.read_bytes() if rows.exists() else None)


@pytest.mark.parametrize("name", ["cascade_break", "paired_mix", "multimap_split"])
def test_map_main_hand_cases(hip, tmp_path, name):
    import os
    cdir = os.path.join(sc.GOLDEN, "cases")
    sam, dbinfo = os.path.join(cdir, name + ".sam"), os.path.join(cdir, "dbinfo.txt")
    with open(sam) as fh:
        want = _definition_bytes(fh.readlines(), dbinfo)
    cami, rows = _run(sam, dbinfo, tmp_path, "with")
    assert rows == want and want.count(b"\n") > 2
    cami0, none = _run(sam, dbinfo, tmp_path, "without", rows=False)
    assert none is None and cami == cami0
    cami_dm, rows_dm = _run(sam, dbinfo, tmp_path, "dm", device_multimap=True)
    assert rows_dm == want


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("assign_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    with open(sam) as fh:
        lines = fh.readlines()
    text = "".join(lines)
    (d / "b.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "b.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    return d, sam, dbinfo, lines, _definition_bytes(lines, dbinfo)


def test_map_main_bulk_as_sam_gz_and_bam(hip, bulk, tmp_path, monkeypatch):
    d, sam, dbinfo, lines, want = bulk
    cami0, _ = _run(sam, dbinfo, tmp_path, "plain", rows=False)
    for tag, path in (("sam", sam), ("gz", d / "b.sam.gz"), ("bam", d / "b.bam")):
        # (--input_type sam: a BAM is recognised by its content; --db only keeps map_main from asking for one, as "x.sam.gz" is no ".sam")
        cami, rows = _run(path, dbinfo, tmp_path, tag, input_type="sam", db="unused.fna")
        assert rows == want, tag
        assert cami == cami0.replace(str(sam), str(path)), tag
    monkeypatch.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))  # many pieces
    assert _run(sam, dbinfo, tmp_path, "pieces")[1] == want
    monkeypatch.setenv("MG_NO_STREAM", "1")  # the whole text, one tokeniser call
    assert _run(sam, dbinfo, tmp_path, "whole")[1] == want


def test_two_input_files_append(hip, bulk, tmp_path):
    d, sam, dbinfo, lines, want = bulk
    out, rows = tmp_path / "two.cami", tmp_path / "two.tsv"
    args = sc.make_args(str(sam), str(dbinfo), str(out), {"input_type": "AUTO", "read_assignments": str(rows)})
    args.infiles = [str(sam), str(d / "b.bam")]
    mp.map_main(args)
    assert rows.read_bytes() == want + want[len(asg.HEADER):]


def test_the_chunked_path_gives_the_same_rows(hip, bulk, tmp_path, monkeypatch):
    d, sam, dbinfo, lines, want = bulk
    monkeypatch.setattr(mp, "_CHUNK_BYTES", 40000)  # many chunks: reads go on from one into the next
    rows = tmp_path / "chunked.tsv"
    args = sc.make_args(str(sam), str(dbinfo), str(tmp_path / "c.cami"), {"read_assignments": str(rows)})
    acc2info, taxid2info = mp.get_acc2info(args)
    asg.write_assignments(str(rows), [])
    with open(sam, "rb") as fh:
        t2a, mm, _ = mp.map_and_process(args, fh, acc2info, taxid2info, _assignments=True)
    assert rows.read_bytes() == want
    with open(sam, "rb") as fh:
        t2a0, mm0, _ = mp.map_and_process(args, fh, acc2info, taxid2info)
    assert t2a == t2a0 and mm == mm0


def test_collated_input_takes_the_definition_over_the_collated_lines(hip, tmp_path):
    import collate_cases as cc
    dbinfo_text, accs, acc_index, text = cc.case(300, 100)
    lines = cc.coordinate_shuffle(text)
    (tmp_path / "db_info.txt").write_text(dbinfo_text)
    (tmp_path / "shuffled.sam").write_text("".join(lines))
    want = _definition_bytes(list(collate.collated_lines(lines)), str(tmp_path / "db_info.txt"))
    cami, rows = _run(tmp_path / "shuffled.sam", tmp_path / "db_info.txt", tmp_path, "col", collate="always")
    assert rows == want and want.count(b"\n") > 100
    cami0, _ = _run(tmp_path / "shuffled.sam", tmp_path / "db_info.txt", tmp_path, "col0", collate="always", rows=False)
    assert cami == cami0
