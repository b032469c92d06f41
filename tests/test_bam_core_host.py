"""The BAM record logic of the device (metalign_amd/csrc/mg_bam_core.h) compiled for the HOST and run on generated BAM streams
(tests/host_bam_check.cpp): the speculative chunk walk + stitch equals the sequential block_size chain at every chunk size of a
sweep, on clean streams and on streams with a corrupt block_size or a cut-off tail; a plausible start is always a record inside
the range; no load leaves the range; and every record decodes to what its SAM rendering (metalign_amd/bam.py) gives through the
host SAM tokeniser.  No GPU needed."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bamgen
import samgen
from metalign_amd import _hip, bam
from metalign_amd import map_and_profile as mp

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [64, 100, 256, 1000, 4096, 65536]
KINDS = {KeyError: 1, IndexError: 2, ValueError: 3, ZeroDivisionError: 4, OverflowError: 5}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bamcore") / "host_bam_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-o", out, os.path.join(HERE, "host_bam_check.cpp")])
    return out


def edge_lines(accs):
    """Hand-built records for the rules of mg_bam_core.h: decode (tests/test_gpu_bam.py uses them too)."""
    a, b = accs[0], accs[1]
    L = samgen._line
    return [
        L("@atq", 0, a, "10M", "ACGTACGTAC", 0),                       # QNAME '@...': a header line, skipped
        L("q" * 254, 0, a, "10M", "ACGTACGTAC", 1),                    # the longest QNAME
        L("r1", 0, a, "4M2I4M", "ACGTACGTAC", 2),
        L("r1", 256, b, "10M", "*", 3),                                 # l_seq 0 (SEQ '*')
        L("r2", 4, "*", "*", "ACGTACGTAC", 0),                          # unmapped
        L("r2", 0, b, "*", "ACGTACGTAC", 0),                            # CIGAR '*'
        "r3\t0\t%s\t1\t60\t10M\t=\t5\t0\tACGTACGTAC\tIIIIIIIIII\tXA:A:7\n" % a,
        "r4\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXZ:Z:12 ab\tNM:i:0\n" % a,
        "r5\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXH:H:12\n" % a,
        "r6\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\t*\tXc:i:-5\n" % a,
        "r7\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXC:i:200\n" % a,
        "r8\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXs:i:-300\n" % a,
        "r9\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXS:i:40000\n" % a,
        "r10\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXi:i:-70000\n" % a,
        "r11\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXI:i:3000000000\n" % a,
        "r12\t0\t%s\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tXf:f:3\n" % a,  # a float tag: the host decides ('3')
    ]


# one record each that the reference cannot parse -> the exception of its SAM rendering
def bad_lines(accs):
    a = accs[0]
    base = "x\t0\t%s\t1\t60\t%s\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII%s\n"
    return [
        ("x\t0\t*\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\n", KeyError),        # refID -1 on a retained record
        (base.replace("%s", "NOPE", 1) % ("10M", "\tNM:i:0"), KeyError),                         # an unknown reference
        (base % (a, "5=5M", "\tNM:i:0"), ValueError),                                            # '=' op
        (base % (a, "0M", "\tNM:i:0"), ZeroDivisionError),
        (base % (a, "10M", ""), IndexError),                                                     # no aux field
        (base % (a, "10M", "\tXA:A:x"), ValueError),
        (base % (a, "10M", "\tXZ:Z:"), ValueError),
        (base % (a, "10M", "\tXH:H:1A"), ValueError),
        (base % (a, "10M", "\tXf:f:2.5"), ValueError),
        (base % (a, "10M", "\tXB:B:c,1,2"), ValueError),
    ]


def _run(exe, tmp_path, stream, names, acc_index, sizes=SIZES):
    refmap = [acc_index.get("*", -1)] + [acc_index.get(n, -1) for n in names]
    p = tmp_path / "in.bin"
    with open(p, "wb") as fh:
        fh.write(struct.pack("<I", len(names)) + struct.pack("<%di" % len(refmap), *refmap) + struct.pack("<Q", len(stream)) + stream
                 + struct.pack("<I", len(sizes)) + struct.pack("<%dI" % len(sizes), *sizes))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.decode().splitlines()
    walks = [ln for ln in lines if ln.startswith("walk ")]
    assert len(walks) == len(sizes) and all(ln.endswith(" ok") for ln in walks), walks
    assert "inside ok" in lines
    end = [ln for ln in lines if ln.startswith("end ")][0].split()
    recs = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("rec ")]
    return int(end[1]), int(end[2]), recs


def _expect(body, names, acc_index):
    """(kind, row or None) of one record by its SAM rendering through the host tokeniser."""
    try:
        line = bam.render(body, [n.encode() for n in names])
    except ValueError:
        return 7, None
    tk = mp._Tokeniser(acc_index)
    try:
        tk.feed(line.decode("utf-8"))
    except tuple(KINDS) as e:
        return KINDS[type(e)], None
    return 0, (tuple(int(x) for x in tk.records()[0]) if tk.rows else None)


def _check_decode(stream, recs, names, acc_index):
    seen_host = 0
    for off, kind, retained, ref_new, matched, total, flag_len, qbeg, qlen in recs:
        (bs,) = struct.unpack_from("<I", stream, off)
        want_kind, want = _expect(stream[off + 4:off + 4 + bs], names, acc_index)
        if kind == 6:  # the device hands the record to the host definition
            seen_host += 1
            continue
        assert kind == want_kind, (off, kind, want_kind)
        if kind == 0:
            assert bool(retained) == (want is not None)
            if want is not None:
                assert (ref_new, matched, total, flag_len) == (want[0] & _hip.REF_MASK, want[1], want[2], want[3])
                assert stream[qbeg:qbeg + qlen] == stream[off + 36:off + 36 + qlen]
    return seen_host


def _case(n=3000, seed=5):
    dbinfo, accs, taxids = samgen.make_dbinfo()
    acc_index = {"Unmapped": 0}
    acc_index.update({x: i + 1 for i, x in enumerate(accs)})
    text = samgen.make_sam_single(seed, n, accs, taxids, readlen=60) + samgen.make_sam_paired(seed + 1, n // 3, accs, taxids)
    return text, accs, acc_index


def test_chunk_walk_and_decode_on_generated_streams(exe, tmp_path):
    text, accs, acc_index = _case()
    lines = text.splitlines(True)
    lines += edge_lines(accs) + [ln for ln, _ in bad_lines(accs)]
    data, hdr, names = bamgen.encode(lines)
    stream = data[hdr:]
    end, status, recs = _run(exe, tmp_path, stream, names, acc_index)
    assert (end, status) == (len(stream), 0)
    assert len(recs) == sum(1 for ln in lines if not ln.startswith("@") or ln.startswith("@atq"))
    assert _check_decode(stream, recs, names, acc_index) == 2  # (the two float tags)


def test_long_read_cg_placeholder_is_refused(exe, tmp_path):
    _, accs, acc_index = _case(10)
    line = "lr\t0\t%s\t1\t60\t10S100N\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tCG:B:I,1600\tNM:i:0\n" % accs[0]
    data, hdr, names = bamgen.encode([line])
    _, _, recs = _run(exe, tmp_path, data[hdr:], names, acc_index)
    assert recs[0][1] == 7
    with pytest.raises(ValueError, match="CG tag"):
        bam.render(data[hdr + 4:], [n.encode() for n in names])


def test_corrupt_and_cut_streams_stitch_like_the_sequential_chain(exe, tmp_path):
    text, accs, acc_index = _case(1500, seed=9)
    data, hdr, names = bamgen.encode(text)
    stream = bytearray(data[hdr:])
    offs, p = [], 0
    while p < len(stream):
        offs.append(p)
        p += 4 + struct.unpack_from("<I", stream, p)[0]
    rng = random.Random(3)
    for trial in range(6):
        s = bytearray(stream)
        victim = offs[rng.randrange(len(offs) // 4, len(offs))]
        struct.pack_into("<I", s, victim, [7, 1 << 31, 0xFFFFFFFF, 40, 1000, 99999][trial])
        cut = len(s) - rng.randrange(0, 400) if trial % 2 else len(s)
        end, status, recs = _run(exe, tmp_path, bytes(s[:cut]), names, acc_index)
        k = offs.index(victim)
        assert status in (1, 2) and [r[0] for r in recs[:k]] == offs[:k]
    # a stream cut in the middle of a record: the chain ends at that record, incomplete
    cut = offs[len(offs) // 2] + 17
    end, status, recs = _run(exe, tmp_path, bytes(stream[:cut]), names, acc_index)
    assert (end, status, len(recs)) == (offs[len(offs) // 2], 1, len(offs) // 2)


def test_bamgen_round_trips_through_the_host_reader(tmp_path):
    text, accs, acc_index = _case(400, seed=11)
    path = tmp_path / "x.bam"
    path.write_bytes(bamgen.sam_to_bam(text, block=1000))
    assert bam.is_bam(str(path)) and bam.has_eof_block(str(path))
    got = list(bam.sam_lines(str(path)))
    want = mp.tokenise_sam(text.splitlines(True), acc_index)
    assert np.array_equal(mp.tokenise_sam(got, acc_index), want) and len(want) > 300
    sam = tmp_path / "x.sam"
    sam.write_text(text)
    assert not bam.is_bam(str(sam))
