"""-m gpu: BAM alignment files decoded on the device (metalign_amd/csrc/mg_bam.hip).

The reference reads SAM text only (/root/reference/scripts/map_and_profile.py:201-217), so BAM has no reference counterpart: parity
is defined THROUGH the SAM path — a BAM must give exactly the records (and so the CAMI profile) that its SAM rendering gives through
the SAM tokeniser, on the device and on the host, the same exceptions on the same record included."""
import random

import numpy as np
import pytest

import bamgen
import samgen
import stage_c_checks as sc
from metalign_amd import _hip, bam
from metalign_amd import map_and_profile as mp
from test_bam_core_host import bad_lines, edge_lines

pytestmark = pytest.mark.gpu

_DEFAULT_INFLATE = dict(chunk_bytes=32 << 10, stage_bytes=-1, ratio=10, on=1, lane_jobs=1 << 40)


@pytest.fixture()
def inflate(hip):
    yield hip.inflate_config
    hip.inflate_config(**_DEFAULT_INFLATE)


def _case(seed=3, nsingle=20000, npairs=4000):
    dbinfo, accs, taxids = samgen.make_dbinfo()
    acc_index = {"Unmapped": 0}
    acc_index.update({a: i + 1 for i, a in enumerate(accs)})
    text = samgen.make_sam_single(seed, nsingle, accs, taxids, readlen=60) + samgen.make_sam_paired(seed + 1, npairs, accs, taxids)
    return dbinfo, accs, acc_index, text


@pytest.mark.parametrize("how", ["device inflater", "host inflater", "device inflater, small pieces", "host inflater, small pieces"])
def test_bam_records_equal_the_sam_records(hip, tmp_path, inflate, how):
    _, accs, acc_index, text = _case()
    want = mp.tokenise_sam(text.splitlines(True), acc_index)
    sam = tmp_path / "x.sam"
    sam.write_text(text)
    assert np.array_equal(mp.tokenise_sam_device(open(str(sam), "rb"), acc_index), want)
    small = "small" in how
    inflate(on=0 if how.startswith("host") else 1)
    if small:
        inflate(chunk_bytes=4 << 10, stage_bytes=64 << 10)
    for block in ((1024, 5000) if small else (65280,)):
        p = tmp_path / ("x_%d.bam" % block)
        p.write_bytes(bamgen.sam_to_bam(text, block=block))
        got = mp.tokenise_bam_device(str(p), acc_index, chunk_bytes=(1 << 16) if small else 0)
        assert len(got) == len(want) > 20000
        assert np.array_equal(got, want), how
        # ... and straight from the library (no host fallback taken)
        idx = hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])
        try:
            b = hip.bam_stream_file(str(p), idx, chunk_bytes=(1 << 16) if small else 0)
            assert b.count == len(want)
            b.free()
        finally:
            idx.free()


def test_bam_tokenize_dev_pieces_carry_the_qname(hip):
    """mg_bam_tokenize_dev on a resident stream cut at arbitrary bytes: consumed = the end of the last whole record, the previous
    QNAME carried — the concatenated records equal one call on the whole stream."""
    _, accs, acc_index, text = _case(seed=7, nsingle=3000, npairs=800)
    data, hdr, names = bamgen.encode(text)
    stream = np.frombuffer(data[hdr:], dtype=np.uint8)
    refmap = np.array([acc_index.get(n, -1) for n in names], dtype=np.int32)
    idx = hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])
    d = hip.array(stream)
    try:
        whole, used = hip.bam_tokenize_dev(d.ptr, stream.size, refmap, idx)
        assert used == stream.size
        want = np.zeros(whole.count, dtype=_hip.REC_DTYPE)
        hip._chk(hip.lib.mg_sam_batch_download(whole.handle, _hip._vp(want.ctypes.data)))
        whole.free()
        assert np.array_equal(want, mp.tokenise_sam(text.splitlines(True), acc_index))
        rng = random.Random(1)
        parts, pos, prev = [], 0, ""
        while pos < stream.size:
            n = min(stream.size - pos, rng.randrange(50, 20000))
            final = pos + n == stream.size
            b, used = hip.bam_tokenize_dev(d.ptr + pos, n, refmap, idx, prev, final=final)
            r = np.zeros(b.count, dtype=_hip.REC_DTYPE)
            if b.count:
                hip._chk(hip.lib.mg_sam_batch_download(b.handle, _hip._vp(r.ctypes.data)))
            prev = b.last_qname
            b.free()
            parts.append(r)
            pos += used
        assert np.array_equal(np.concatenate(parts), want)
        with pytest.raises(_hip.SamParseError) as e:  # the last record cut: a truncated stream
            hip.bam_tokenize_dev(d.ptr, stream.size - 3, refmap, idx)
        assert e.value.kind == 7
    finally:
        d.free()
        idx.free()


def test_map_main_on_a_bam_writes_the_sam_profile(hip, tmp_path):
    dbinfo_text, accs, acc_index, text = _case(seed=5, nsingle=20000, npairs=3000)
    dbinfo = tmp_path / "db_info.txt"
    dbinfo.write_text(dbinfo_text)
    sam, bm = tmp_path / "x.sam", tmp_path / "x.bam"
    sam.write_text(text)
    bm.write_bytes(bamgen.sam_to_bam(text, block=20000))
    outs = {}
    for name, infiles, extra in (("sam", [sam], {}), ("bam", [bm], {}), ("bam_dm", [bm], {"device_multimap": True}),
                                 ("mixed", [bm, sam], {}), ("mixed_ref", [sam, sam], {})):
        out = tmp_path / (name + ".tsv")
        args = sc.make_args(str(infiles[0]), str(dbinfo), str(out), dict({"input_type": "AUTO", "sampleID": "s"}, **extra))
        args.infiles = [str(f) for f in infiles]
        mp.map_main(args)
        outs[name] = out.read_text()
    assert outs["bam"] == outs["sam"] and outs["sam"].count("\n") > 20
    assert outs["mixed"] == outs["mixed_ref"]
    a = [ln.split("\t") for ln in outs["sam"].splitlines() if ln and ln[0] != "@"]
    b = [ln.split("\t") for ln in outs["bam_dm"].splitlines() if ln and ln[0] != "@"]
    assert [r[0] for r in a] == [r[0] for r in b]
    assert all(abs(float(x[4]) - float(y[4])) <= 1e-6 for x, y in zip(a, b))
    # --input_type sam with a BAM that does not say so in its name
    out = tmp_path / "named.tsv"
    other = tmp_path / "mislabelled.sam"  # (a BAM by its bytes)
    other.write_bytes(bm.read_bytes())
    mp.map_main(sc.make_args(str(other), str(dbinfo), str(out), {"input_type": "sam", "sampleID": "s"}))
    assert out.read_text() == outs["sam"]


def test_hand_built_records(hip, tmp_path, capsys):
    _, accs, acc_index, _ = _case(nsingle=10, npairs=0)
    head = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:UNUSED.1\tLN:10\n"
    good = head + "".join(edge_lines(accs))
    p = tmp_path / "edges.bam"
    p.write_bytes(bamgen.sam_to_bam(good, block=300))
    want = mp.tokenise_sam(good.splitlines(True), acc_index)
    assert len(want) == 13
    assert np.array_equal(mp.tokenise_bam_device(str(p), acc_index), want)
    assert np.array_equal(mp.tokenise_sam(list(bam.sam_lines(str(p))), acc_index), want)
    bam.warn_about(str(p))
    assert "sorted by coordinate" in capsys.readouterr().err
    for line, exc in bad_lines(accs):
        text = good + line + "".join(edge_lines(accs))
        with pytest.raises(exc):
            mp.tokenise_sam(text.splitlines(True), acc_index)
        q = tmp_path / "bad.bam"
        q.write_bytes(bamgen.sam_to_bam(text, block=500))
        with pytest.raises(exc):
            mp.tokenise_bam_device(str(q), acc_index)
    # the long-read placeholder CIGAR (the real one in CG:B,I) is refused with a clear error
    q = tmp_path / "cg.bam"
    q.write_bytes(bamgen.sam_to_bam(good + "lr\t0\t%s\t1\t60\t10S100N\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tCG:B:I,1600\n" % accs[0]))
    with pytest.raises(ValueError, match="CG tag"):
        mp.tokenise_bam_device(str(q), acc_index)


def test_broken_files_end_in_a_clean_exception(hip, tmp_path, capsys):
    _, accs, acc_index, text = _case(seed=9, nsingle=3000, npairs=0)
    data, hdr, names = bamgen.encode(text)
    offs, p = [], hdr
    while p < len(data):
        offs.append(p)
        p += 4 + int.from_bytes(data[p:p + 4], "little")
    cut = tmp_path / "cut.bam"  # truncated in the middle of a record (whole BGZF members)
    cut.write_bytes(bamgen.bgzf(data[:offs[len(offs) // 2] + 50], block=4000))
    with pytest.raises(ValueError, match="cut.bam"):
        mp.tokenise_bam_device(str(cut), acc_index)
    bad = bytearray(data)  # one corrupt block_size
    bad[offs[len(offs) // 3]:offs[len(offs) // 3] + 4] = (40).to_bytes(4, "little")
    cor = tmp_path / "corrupt.bam"
    cor.write_bytes(bamgen.bgzf(bytes(bad), block=4000))
    with pytest.raises(ValueError, match="corrupt.bam"):
        mp.tokenise_bam_device(str(cor), acc_index)
    noeof = tmp_path / "noeof.bam"  # no BGZF end-of-file block: accepted, with a warning
    noeof.write_bytes(bamgen.bgzf(data, block=4000, eof=False))
    assert np.array_equal(mp.tokenise_bam_device(str(noeof), acc_index), mp.tokenise_sam(text.splitlines(True), acc_index))
    bam.warn_about(str(noeof))
    assert "end-of-file" in capsys.readouterr().err


def test_full_size_bam_equals_bgzf_sam(hip, tmp_path):
    """>= 2 M alignment records: the BAM and the BGZF SAM of the same lines give the same records."""
    _, accs, acc_index, _ = _case(nsingle=10, npairs=0)
    rng = random.Random(4)
    lines = []
    for r in range(6700):  # a primary and two secondaries per read, x 100 below
        k = rng.randrange(20, 41)
        cig = "40M" if k == 40 else "%dM%dS" % (k, 40 - k)
        lines.append(samgen._line("r%d" % r, rng.choice((0, 16)), rng.choice(accs), cig, samgen._seq(rng, 40), k & 7))
        for _ in range(2):
            lines.append(samgen._line("r%d" % r, 256, rng.choice(accs), cig, "*", 1))
    data, hdr, _ = bamgen.encode(lines)
    rep = 100
    sgz, bm = tmp_path / "big.sam.gz", tmp_path / "big.bam"
    sgz.write_bytes(bamgen.bgzf("".join(lines).encode() * rep, level=1))
    bm.write_bytes(bamgen.bgzf(data[:hdr] + data[hdr:] * rep, level=1))
    n = len(lines) * rep
    idx = hip.acc_index([a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])])
    try:
        a = hip.sam_stream_file(str(sgz), idx)
        b = hip.bam_stream_file(str(bm), idx)
        assert a.count == b.count == n >= 2_000_000
        ra, rb = np.zeros(n, _hip.REC_DTYPE), np.zeros(n, _hip.REC_DTYPE)
        hip._chk(hip.lib.mg_sam_batch_download(a.handle, _hip._vp(ra.ctypes.data)))
        hip._chk(hip.lib.mg_sam_batch_download(b.handle, _hip._vp(rb.ctypes.data)))
        a.free()
        b.free()
    finally:
        idx.free()
    assert np.array_equal(ra, rb)
