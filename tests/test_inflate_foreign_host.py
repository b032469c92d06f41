"""CPU: the inflaters against zlib's INFLATER on DEFLATE streams zlib's compressor never writes (tests/deflate_writer.py assembles them:
distances up to 32768, one distance code of one bit, no distance code, codes of every shape, headers as no encoder sends them, blocks of
a million symbols, false block starts carried in stored blocks, two hundred random legal streams; and streams that must be refused).
The decoder of the device inflater as the host compiles it (tests/host_inflate_check.cpp: whole streams by both decoders, jobs entered at
the starts either pass of the finder reports) and the library's threaded host inflater (mg_pgzip.hip).  tests/test_gpu_inflate_foreign.py
runs the same corpus on the device."""
import os
import re
import struct
import subprocess
import zlib

import pytest

import deflate_writer as dw
from metalign_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
# the named cases that have no BGZF form: more than one member, or more than a BGZF block holds (64 KB of text)
NO_BGZF_FORM = [
    "second member, distance exactly the member's bytes", "second BGZF block, distance exactly the member's bytes",
    "second member, distance into the previous member", "second BGZF block, distance into the previous member",
    "second member, distance far into the previous member", "second BGZF block, distance far into the previous member",
    "255 matches, each a copy of the one before (258 bytes each)", "length-258 matches around the boundary of the 4096-byte batch",
    "jobs entered at a block whose first symbol copies window bytes 0 and 32767",
    "legal headers no encoder writes, megabytes of them (the finder's second pass)", "stored blocks of 0 and 65535 bytes",
    "one dynamic block of a million symbols", "megabytes of fixed and stored blocks only",
    "a whole .gz carried in stored blocks: every block start in it is a false one",
]
# the named cases of the corpus, in its order: (name, zlib reads it)
NAMED = [
    ('every distance symbol, smallest and largest extra bits (fixed)', True),
    ('distance 32506', True),
    ('distance 32507', True),
    ('distance 32767', True),
    ('distance 32768', True),
    ('distance = the 1 bytes there are', True),
    ('distance one more than the 1 bytes there are', False),
    ('distance = the 2 bytes there are', True),
    ('distance one more than the 2 bytes there are', False),
    ('distance = the 257 bytes there are', True),
    ('distance one more than the 257 bytes there are', False),
    ('distance = the 4096 bytes there are', True),
    ('distance one more than the 4096 bytes there are', False),
    ('distance = the 32768 bytes there are', True),
    ('a match as the first symbol', False),
    ('too far, dynamic block, after a stored block', False),
    ("second member, distance exactly the member's bytes", True),
    ("second BGZF block, distance exactly the member's bytes", True),
    ('second member, distance into the previous member', False),
    ('second BGZF block, distance into the previous member', False),
    ('second member, distance far into the previous member', False),
    ('second BGZF block, distance far into the previous member', False),
    ('copies of distance 1 to 8, lengths up to 258', True),
    ('255 matches, each a copy of the one before (16 bytes each)', True),
    ('255 matches, each a copy of the one before (7 bytes each)', True),
    ('255 matches, each a copy of the one before (1 bytes each)', True),
    ('255 matches, each a copy of the one before (258 bytes each)', True),
    ('length-258 matches around the boundary of the 4096-byte batch', True),
    ('length-258 matches around the boundary of the 256-symbol batch', True),
    ('jobs entered at a block whose first symbol copies window bytes 0 and 32767', True),
    ('every length symbol, smallest and largest extra bits', True),
    ('length 258 both ways', True),
    ('a literal/length code of every length 1 to 15', True),
    ('frequent symbols with codes of 11 to 15 bits', True),
    ('distance codes of 9 to 15 bits', True),
    ('literal codes of 1 to 4 bits, distance codes of 1 and 2 bits', True),
    ('all 286 literal/length and all 30 distance symbols in use', True),
    ('one distance code of one bit: matches through it', True),
    ('one distance code of one bit: distance symbol 0', True),
    ('one distance code of one bit: the unassigned bit pattern', False),
    ('no distance code: all literals', True),
    ('no distance code: a match', False),
    ('only the end-of-block symbol, one bit, in an empty dynamic block', True),
    ('an empty dynamic block in front of text', True),
    ('fixed block, literal/length symbol 286', False),
    ('fixed block, literal/length symbol 287', False),
    ('fixed block, distance symbol 30', False),
    ('fixed block, distance symbol 31', False),
    ('a run of symbol 16 that crosses from the literal/length into the distance lengths', True),
    ('a run of symbol 18 that crosses from the literal/length into the distance lengths', True),
    ('symbol 16 as the first code-length symbol', False),
    ('a run that passes the end of the length list', False),
    ('a run of symbol 16 that passes the end of the length list', False),
    ('an incomplete code-length code', False),
    ('an over-subscribed code-length code', False),
    ('no end-of-block symbol', False),
    ('an over-subscribed literal/length code', False),
    ('an incomplete literal/length code', False),
    ('an incomplete distance code of two symbols', False),
    ('an incomplete distance code: one symbol of two bits', False),
    ('an over-subscribed distance code', False),
    ('HLIT 30', False),
    ('HLIT 31', False),
    ('HDIST 30', False),
    ('HDIST 31', False),
    ('block type 3', False),
    ('block type 3 after a good block', False),
    ("legal headers no encoder writes, megabytes of them (the finder's second pass)", True),
    ('stored blocks at all eight bit alignments, padding bits set', True),
    ('stored blocks of 0 and 65535 bytes', True),
    ('a stored block with a bad NLEN', False),
    ('a stored block with a bad NLEN after text', False),
    ('a thousand empty fixed blocks', True),
    ('a thousand dynamic blocks of one symbol', True),
    ('one dynamic block of a million symbols', True),
    ('megabytes of fixed and stored blocks only', True),
    ('a final stored block at the start', True),
    ('a final fixed block at the start', True),
    ('a final dynamic block at the start', True),
    ('header fields', True),
    ('a whole .gz carried in stored blocks: every block start in it is a false one', True),
]


@pytest.fixture(scope="module")
def entries():
    e = dw.corpus()
    return e + dw.bgzf_forms(e)


@pytest.fixture(autouse=True)
def _knobs_back():
    yield
    _hip.debug_set(None)


def test_the_writer_agrees_with_zlib_and_with_itself(entries):
    """Every legal stream: zlib's inflater and expand() give the same text (corpus() compared them; once more here, counted); every illegal
    one: zlib refuses the DATA, not a trailer.  And the stream of the issue that started this: 32768 literals, then 258 bytes from 32768
    back — both codings of the length — is read by zlib; one literal fewer and it is refused."""
    legal = refused = 0
    for e in entries:
        if e.want is None:
            with pytest.raises(zlib.error) as err:
                dw.zlib_inflate(e.blob)
            assert "incorrect" not in str(err.value), e.name
            refused += 1
        else:
            assert dw.zlib_inflate(e.blob) == e.want, e.name
            legal += 1
    # the corpus is seeded: every named case is there under its name, with zlib's verdict, then the 200 random streams; 138 of the 281 fit a
    # BGZF block and have a BGZF form — 419 files, 353 legal and 66 refused, 188 of them BGZF
    first = entries[:281]
    assert [(e.name, e.want is not None) for e in first[:len(NAMED)]] == NAMED
    assert [e.name for e in first[len(NAMED):]] == ["random %d" % i for i in range(200)] and all(e.want is not None for e in first[len(NAMED):])
    forms = entries[281:]
    assert len(forms) == 138 and all(e.name.startswith("BGZF: ") and e.bgzf for e in forms)
    assert {n for n, _ in NAMED} - {e.name[6:] for e in forms} == set(NO_BGZF_FORM)
    assert (len(entries), legal, refused, sum(e.bgzf for e in entries)) == (419, 353, 66, 188), (len(entries), legal, refused)
    assert sum(len(e.blob) for e in entries) == 7_229_263 and sum(len(e.want) for e in entries if e.want is not None) == 19_421_167
    # the decoder's batch sizes, which the two batch-boundary cases are laid around, are the core's
    core = open(os.path.join(os.path.dirname(HERE), "metalign_amd", "csrc", "mg_inflate_core.h")).read()
    assert int(re.search(r"constexpr uint32_t kBatchBytes = (\d+);", core).group(1)) == dw.kBatchBytes
    assert int(re.search(r"constexpr uint32_t kBatchSyms = (\d+);", core).group(1)) == dw.kBatchSyms
    assert sum(len(e.blob) > 700_000 for e in entries) >= 3  # (the streams that span many chunks and several stages)
    lits = bytes(range(256)) * 128
    for alt in (False, True):
        s = dw.Stream().fixed([lits, (258, 32768, alt)], True)
        assert zlib.decompress(s.raw(), -15) == lits + lits[:258] == s.data()
        with pytest.raises(zlib.error, match="too far back"):
            zlib.decompress(dw.Stream().fixed([lits[1:], (258, 32768, alt)], True).raw(), -15)
    # the bit writer against zlib's own deflater where the two can be compared: a stored block, bit for bit
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    assert dw.Stream().stored(b"stored", True).raw() == co.compress(b"stored") + co.flush()
    # what the writer is asked for is what it sends
    s = dw.Stream().dynamic([65], dw.spread(257, [65, 256], [1, 1]), [0], True, hlit=280, hdist=7, hclen=19)
    head = int.from_bytes(s.raw()[:3], "little")
    assert head & 7 == 5 and (head >> 3) & 31 == 280 - 257 and (head >> 8) & 31 == 6 and (head >> 13) & 15 == 15
    assert dw.kraft(dw.flat_code(286)) == 32768 and dw.canonical([2, 1, 3, 3]) == [0b01, 0b0, 0b011, 0b111]


def test_the_decoder_as_the_host_compiles_it_reads_what_zlib_reads(entries, tmp_path):
    exe = str(tmp_path / "host_inflate_check")
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-o", exe, os.path.join(HERE, "host_inflate_check.cpp"), "-lz"])
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        for e in entries:
            name = e.name.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<BI", e.want is not None, e.members))
            f.write(struct.pack("<Q", len(e.blob)) + e.blob + struct.pack("<Q", len(e.want or b"")) + (e.want or b""))
    out = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    text = out.stdout[-2000:].decode("utf-8", "replace")
    assert out.returncode == 0 and out.stdout.startswith(b"ok "), text
    m = re.match(r"ok (\d+) checks, (\d+) legal streams, (\d+) refused, (\d+) jobs entered in the middle by the finder's first pass, (\d+) by its second, (\d+) bytes", text)
    legal = [e for e in entries if e.want is not None]
    assert m and int(m.group(2)) == len(legal) == 353 and int(m.group(3)) == len(entries) - len(legal) == 66, text
    # (the program holds each pass to the block starts it owes; here only that each pass did enter jobs, and as many as before together)
    first_pass, second_pass = int(m.group(4)), int(m.group(5))
    assert int(m.group(6)) == sum(len(e.want) for e in legal) and first_pass > 0 and second_pass > 0 and first_pass + second_pass > 300, text
    print(text)


@pytest.mark.parametrize("threads,chunk", [(1, 4 << 10), (4, 8 << 10), (6, 20_000)])
def test_the_threaded_host_inflater_reads_what_zlib_reads(entries, tmp_path, threads, chunk):
    _hip.debug_set("pgzip_chunk", chunk)
    p = str(tmp_path / "a.gz")
    legal = refused = 0
    for e in entries:
        with open(p, "wb") as f:
            f.write(e.blob)
        if e.want is None:
            with pytest.raises(OSError):
                _hip.gunzip_file(p, nthreads=threads)
            refused += 1
        else:
            got = _hip.gunzip_file(p, nthreads=threads, piece=8 << 20)
            assert len(got) == len(e.want) and got == e.want, e.name
            legal += 1
    assert legal + refused == len(entries) and refused == sum(e.want is None for e in entries)
