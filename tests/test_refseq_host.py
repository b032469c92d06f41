"""CPU: metalign_amd/refseq.py (the reference bases per accession from FASTA bytes) against hand-worked texts, and
mg_refseq_core.h — the per-byte, per-line and per-record rules — on the host under the sanitizers."""
import gzip
import os
import struct
import subprocess

import pytest

import refdiff_cases as rc
from metalign_amd import refseq as rs

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hand_table_records_kinds_and_codes():
    assert rs.records_of(rc.HAND_TEXT) == rc.HAND_RECORDS
    got = rs.parse(rc.HAND_TEXT, rc.HAND_INDEX, rc.HAND_LENGTHS)
    assert got.codes == rc.HAND_CODES and got.loaded == rc.HAND_LOADED and tuple(got.counters) == rc.HAND_COUNTERS
    assert sum(got.counters[1:]) == got.counters.records
    assert rs.flat(got, rc.HAND_LENGTHS) == b"\xff" * 4 + bytes([0, 4, 2]) + b"\xff" * 7
    # names given as bytes are the same rows
    assert rs.parse(rc.HAND_TEXT, {k.encode(): v for k, v in rc.HAND_INDEX.items()}, rc.HAND_LENGTHS) == got


@pytest.mark.parametrize("white", [b" ", b"\t", b"\r", b"\v", b"\f"])
def test_a_name_ends_at_each_of_the_five_white_bytes_and_nowhere_else(white):
    assert rs.name_of(b">acc.1" + white + b"rest") == b"acc.1" and rs.name_of(b">" + white + b"acc") == b""
    assert rs.name_of(b">acc|1:x;y\x00z\x1c") == b"acc|1:x;y\x00z\x1c" and rs.name_of(b">") == b""
    got = rs.parse(b">r" + white + b"x\n" + white + b"AC" + white + b"GT" + white + white + b"\n", {"r": 0}, [5])
    assert got.codes == {0: bytes([0, 1, 4, 2, 3])}  # stripped at both ends; the one inside stays and is OTHER


def test_codes_lower_case_and_every_other_byte():
    assert rs.codes_of(b"ACGTacgtNnRYKM*-.>\x00\xff") == bytes([0, 1, 2, 3, 0, 1, 2, 3] + [4] * 12)


EDGE_WANT = {
    "empty": ((0, 0, 0, 0, 0), {}),
    "newline_only": ((0, 0, 0, 0, 0), {}),
    "no_header": ((0, 0, 0, 0, 0), {}),
    "headers_only": ((4, 1, 1, 2, 0), {0: b""}),  # r0 has length 0: loaded; r1 and r2 lack their bases
    "header_last_line": ((2, 2, 0, 0, 0), {0: b"", 1: bytes([0, 1, 2, 3, 0, 1])}),
    "header_last_line_newline": ((2, 2, 0, 0, 0), {0: b"", 1: bytes([0, 1, 2, 3, 0, 1])}),
    "no_final_newline": ((1, 1, 0, 0, 0), {1: bytes([0, 1, 2, 3, 0, 1])}),
    "crlf": ((2, 2, 0, 0, 0), {1: bytes([0, 1, 2, 3, 0, 1]), 2: bytes([0, 1])}),
    "one_line_each": ((3, 3, 0, 0, 0), {0: b"", 1: bytes([0, 1, 2, 3, 0, 1]), 2: bytes([0, 1])}),
}


@pytest.mark.parametrize("name", sorted(rc.EDGE_TEXTS))
def test_edge_texts(name):
    index = {a: i for i, a in enumerate(rc.EDGE_NAMES)}
    got = rs.parse(rc.EDGE_TEXTS[name], index, rc.EDGE_LENGTHS)
    counters, codes = EDGE_WANT[name]
    assert tuple(got.counters) == counters and got.codes == codes and got.loaded == [int(r in codes) for r in range(3)]


def test_the_geometry_generator_holds_every_kind_between_loaded_records():
    for width in rc.LINE_WIDTHS:
        text, names, lens = rc.geometry(width)
        got = rs.parse(text, {a: i for i, a in enumerate(names)}, lens)
        assert tuple(got.counters) == (14, 10, 1, 1, 2), width
        assert got.loaded == [1] * 10 + [0] and [len(got.codes[r]) for r in range(10)] == rc.RECORD_LENGTHS
        assert len(set(got.codes[9])) == 5
    # lines of 16 bases and their newline: the newlines fall in every byte of a 16-byte window
    assert {i % 16 for i, b in enumerate(rc.geometry(16)[0]) if b == 10} == set(range(16))


def test_read_bytes_inflates_gzip_by_its_magic(tmp_path):
    (tmp_path / "r.fa").write_bytes(rc.HAND_TEXT)
    (tmp_path / "r.fa.gz").write_bytes(gzip.compress(rc.HAND_TEXT[:100]) + gzip.compress(rc.HAND_TEXT[100:]))  # two members
    assert rs.read_bytes(str(tmp_path / "r.fa")) == rs.read_bytes(str(tmp_path / "r.fa.gz")) == rc.HAND_TEXT


# ---- mg_refseq_core.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("refseq") / "host_refdiff_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_refdiff_check.cpp")])
    return out


def text_case(text, names, lengths):
    """A text beside what refseq.py says of it, as tests/host_refdiff_check.cpp reads it."""
    want = rs.parse(text, {a: i for i, a in enumerate(names)}, lengths)
    blob = struct.pack("<II", len(text), len(names)) + struct.pack("<%dQ" % len(lengths), *lengths)
    for a in names:
        blob += struct.pack("<I", len(a.encode())) + a.encode()
    return blob + text + struct.pack("<5Q", *want.counters) + bytes(want.loaded) + rs.flat(want, lengths)


def run_check(exe, tmp_path, texts, sites=()):
    p = tmp_path / "cases.bin"
    p.write_bytes(struct.pack("<I", len(texts)) + b"".join(texts) + struct.pack("<I", len(sites)) + b"".join(sites))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.decode().splitlines()[-1] == "%d texts, %d sites, 0 differ" % (len(texts), len(sites))


def test_core_header_against_the_definition(exe, tmp_path):
    names = sorted(rc.HAND_INDEX, key=rc.HAND_INDEX.get)
    texts = [text_case(rc.HAND_TEXT, names, rc.HAND_LENGTHS)]
    texts += [text_case(t, rc.EDGE_NAMES, rc.EDGE_LENGTHS) for t in rc.EDGE_TEXTS.values()]
    texts += [text_case(*rc.geometry(w)) for w in rc.LINE_WIDTHS]
    # every prefix of the hand table: a text that ends inside a header, a name, a line, behind a \r
    texts += [text_case(rc.HAND_TEXT[:n], names, rc.HAND_LENGTHS) for n in range(len(rc.HAND_TEXT))]
    assert len(texts) == 1 + len(rc.EDGE_TEXTS) + len(rc.LINE_WIDTHS) + len(rc.HAND_TEXT) and len(rc.HAND_TEXT) > 100
    run_check(exe, tmp_path, texts)
