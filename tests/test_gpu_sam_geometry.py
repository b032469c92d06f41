"""-m gpu: the SAM / PAF tokenisers of mg_ingest.hip held to their definition wherever the bytes lie (tests/sam_cases.py): the
line index at every misalignment of the text against its 16-byte windows, fields that start and end on every residue of the 8-byte
scan, every field count and error, QNAMEs around the 16-lane gather and the carried name, more lines than one pass of the grid,
and the same text through the file reader's unaligned pieces.  Equality with sam_cases.expected is exact everywhere.

The text is uploaded between pads of '\\n' and separator bytes, `mis` bytes in front and 32 behind: a kernel that looks outside
[0, nbytes) finds line ends and field ends there, and the answer changes."""
import functools
import gzip
import itertools
import re
from collections import namedtuple

import numpy as np
import pytest

import sam_cases as sc
from metalign_amd import _hip
from metalign_amd import map_and_profile as mp

pytestmark = pytest.mark.gpu

FRONT = b"\n\t \n\x0b\n\x0c\r\n\x1c\x1d\n\x1e\x1f\n\n"   # (the text starts behind its last `mis` bytes)
BACK = b"\t\n \n\x1f\n\r\n" * 4
FLAGS = ("named", "keyed", "placed", "edited", "based")
COMBOS = [dict(zip(FLAGS, bits)) for bits in itertools.product((False, True), repeat=5) if any(bits)]
FAMILIES = {"window_edges": sc.window_edges(), "field_alignment": sc.field_alignment(), "qnames": sc.qnames()}
Got = namedtuple("Got", "recs last_qname names keys places edits bases error")


@pytest.fixture(scope="module")
def index(hip):
    ix = hip.acc_index(sc.NAMES)
    yield ix
    ix.free()


LAZY = {"field_counts": sc.field_counts, "paf_fields": sc.paf_fields, "window_edges_paf": functools.partial(sc.window_edges, True)}


@functools.lru_cache(maxsize=None)
def _cases(family):
    return FAMILIES[family] if family in FAMILIES else LAZY[family]()


@functools.lru_cache(maxsize=None)
def _want(family, i, prev="", paf=False):
    """The definition over case i of a family: computed once, shared by every test that needs it."""
    return sc.expected(_cases(family)[i][1], sc.IDX, prev, paf)


def _upload(hip, text, mis):
    """-> the device array; the text lies at .ptr + mis."""
    assert 0 <= mis < 16 and len(FRONT) == 16 and len(BACK) == 32
    d = hip.array(np.frombuffer(FRONT[16 - mis:] + bytes(text) + BACK, dtype=np.uint8))
    assert d.ptr % 16 == 0  # (so `mis` is the text's address modulo 16)
    return d


def _tokenise(hip, index, d, mis, nbytes, prev="", paf=False, **flags):
    try:
        batch = hip.sam_tokenize_dev_batch(d.ptr + mis, nbytes, index, prev, paf=paf, **flags)
    except _hip.SamParseError as e:
        return Got(None, None, None, None, None, None, None, (e.kind, e.line))
    try:
        return Got(batch.download(), batch.last_qname, batch.names() if flags.get("named") else None,
                   batch.keys() if flags.get("keyed") else None, batch.places() if flags.get("placed") else None,
                   batch.edits() if flags.get("edited") else None, batch.bases() if flags.get("based") else None, None)
    finally:
        batch.free()


def _same(got, want, text, paf=False, what=None):
    if want.error is not None:
        exc, message, line = want.error
        assert got.error == (sc.KIND_OF[exc], line), what
        # what tokenise_sam_device does with the line the device names: the host statement over it raises, type and message
        bad = bytes(text).split(b"\n")[got.error[1]].decode("utf-8", "replace")
        with pytest.raises(exc) as e:
            if paf:
                mp.tokenise_paf([bad], sc.IDX)
            else:
                mp._Tokeniser(sc.IDX).feed(bad)
        assert str(e.value) == message, what
        return
    assert got.error is None, (what, got.error)
    assert np.array_equal(got.recs, want.recs), what  # (the new-read bit is bit 31 of ref_new)
    assert got.last_qname == want.last_qname, what
    if got.names is not None:
        assert got.names[0] == want.names[0] and np.array_equal(got.names[1], want.names[1]), what
    if got.keys is not None:  # one key per name: equal names, equal keys, and no others
        k = [tuple(row) for row in got.keys.tolist()]
        assert len(k) == len(want.qnames) and len(set(k)) == len(set(want.qnames)) == len(set(zip(k, want.qnames))), what
    if got.places is not None:
        assert np.array_equal(got.places, want.places), what
    if got.edits is not None:
        assert np.array_equal(got.edits, want.edits), what
    if got.bases is not None:
        assert np.array_equal(got.bases[0], want.bases[0]) and got.bases[1] == want.bases[1], what


def _prevs(family, text):
    return sc.prev_qnames(text) if family == "qnames" else [""]


@pytest.mark.parametrize("mis", range(16))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_plain_calls_at_every_misalignment(hip, index, family, mis):
    for i, (name, text) in enumerate(FAMILIES[family]):
        d = _upload(hip, text, mis)
        try:
            for prev in _prevs(family, text):
                _same(_tokenise(hip, index, d, mis, len(text), prev), _want(family, i, prev), text, what=(name, prev[-8:]))
        finally:
            d.free()


@pytest.mark.parametrize("mis", [0, 1, 7, 8, 9, 15])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_combination_of_batch_flags(hip, index, family, mis):
    """named, keyed, placed, edited, based in all 31 combinations; edited and based take k_sam_parse<true>, whose records are the
    plain call's."""
    assert len(COMBOS) == 31
    for i, (name, text) in enumerate(FAMILIES[family]):
        d = _upload(hip, text, mis)
        try:
            for prev in _prevs(family, text):
                want = _want(family, i, prev)
                plain = _tokenise(hip, index, d, mis, len(text), prev)
                for flags in COMBOS:
                    got = _tokenise(hip, index, d, mis, len(text), prev, **flags)
                    _same(got, want, text, what=(name, prev[-8:], flags))
                    if want.error is None:
                        assert np.array_equal(got.recs, plain.recs) and got.last_qname == plain.last_qname
                    else:
                        assert got.error == plain.error
        finally:
            d.free()


@pytest.mark.parametrize("edited", [False, True])
@pytest.mark.parametrize("mis", [0, 5])
def test_field_counts_and_errors(hip, index, mis, edited):
    """Every field count and every error kind, alone and in pairs; a retained line of 6 to 9 fields is the definition's IndexError
    (its SEQ field does not exist: the parser must not look for it)."""
    cases = _cases("field_counts")
    flags = {"edited": True} if edited else {}
    for i, (name, text) in enumerate(cases):
        d = _upload(hip, text, mis)
        try:
            _same(_tokenise(hip, index, d, mis, len(text), **flags), _want("field_counts", i), text, what=name)
        finally:
            d.free()


def test_more_lines_than_one_pass_of_the_grid(hip, index):
    ncu = int(re.search(r"(\d+) CUs\)", hip.device_name()).group(1))
    assert ncu > 0
    text, where = sc.many_lines(ncu)
    grid = sc.grid_lines(ncu)
    want = sc.expected(text, sc.IDX)
    k = where.index(grid)
    assert text.count(b"\n") == grid + 100000 and len(want.recs) == len(where) and want.qnames[k - 1] == want.qnames[k]
    mis = 3
    d = _upload(hip, text, mis)
    try:
        _same(_tokenise(hip, index, d, mis, len(text), named=True), want, text)
    finally:
        d.free()


@pytest.mark.parametrize("mis", [0, 5, 15])
def test_paf_lines(hip, index, mis):
    for family in ("paf_fields", "window_edges_paf"):
        for i, (name, text) in enumerate(_cases(family)):
            want = _want(family, i, "", True)
            d = _upload(hip, text, mis)
            try:
                for flags in ({}, {"named": True}, {"keyed": True}, {"named": True, "keyed": True}):
                    _same(_tokenise(hip, index, d, mis, len(text), paf=True, **flags), want, text, paf=True, what=(name, flags))
            finally:
                d.free()


def _stream_text():
    """field_alignment and qnames text, repeated over more than four 64 KiB pieces of a file; around every multiple of 64 KiB the
    lines share ONE name, so wherever the reader cuts there the carried QNAME decides the new-read bit."""
    body = b"".join(t for _, t in FAMILIES["field_alignment"]) + b"".join(t for _, t in FAMILIES["qnames"])
    same = sc.sam_line("carried" * 3, 16, "X5abc", 77, cigar="3M2I4M", seq="ACGTACGTA", qual="IIIIIIIII", tags=("XS:i:4", "NM:i:2")) + b"\n"
    buf = bytearray()
    for k in range(1, 5):
        edge = k << 16
        while len(buf) + len(body) <= edge - 1024:
            buf += body
        while len(buf) < edge + 256:
            buf += same
    buf += body
    return bytes(buf)


@pytest.mark.parametrize("gz", [False, True])
def test_through_the_file_reader_in_pieces_of_64_kib(hip, index, tmp_path, gz):
    text = _stream_text()
    assert len(text) > 4 << 16
    for k in range(1, 5):  # the last line end in front of every multiple of 64 KiB lies between two lines of one name
        cut = text.rfind(b"\n", 0, k << 16) + 1
        assert text[cut:cut + 7] == b"carried" and text[:cut].endswith(text[cut:text.index(b"\n", cut) + 1])
    want = sc.expected(text, sc.IDX)
    assert want.error is None and len(want.recs) > 1500 and len(set(want.qnames)) > 50
    path = tmp_path / ("s.sam.gz" if gz else "s.sam")
    path.write_bytes(gzip.compress(text, 6) if gz else text)
    for flags in ({}, {"named": True}, {"named": True, "placed": True, "edited": True, "based": True}):
        batch = hip.sam_stream_file(str(path), index, chunk_bytes=1 << 16, **flags)
        try:
            got = Got(batch.download(), batch.last_qname, batch.names() if flags.get("named") else None, None,
                      batch.places() if flags.get("placed") else None, batch.edits() if flags.get("edited") else None,
                      batch.bases() if flags.get("based") else None, None)
        finally:
            batch.free()
        _same(got, want, text, what=flags)
