"""The case table of tests/sam_cases.py reaches what it claims (so that a later edit cannot empty a family silently), expected() adds
nothing but the splitting rule, and the three known departures are what DESIGN.md says they are.  No GPU."""
import numpy as np
import pytest

import sam_cases as sc
import samgen
from metalign_amd import coverage as cv
from metalign_amd import map_and_profile as mp


def _newlines(text):
    return np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 0x0A)


def test_window_edges_put_a_newline_on_every_byte_of_a_window_at_every_misalignment():
    for paf in (False, True):
        cases = sc.window_edges(paf)
        short = [t for _, t in cases if len(t) <= 48]
        long = [t for _, t in cases if len(t) > 2 * 4096]
        assert len(short) + len(long) == len(cases) and len(long) >= 3 and {len(t) for t in short} >= set(range(0, 49, 16)) | {1, 48}
        for group in (short, long):
            for mis in range(16):
                assert {int(o + mis) % 16 for t in group for o in _newlines(t)} == set(range(16)), (paf, mis)
        # first and last byte of a text, text of newlines only, none at all, with and without a final one, CRLF
        assert any(t[:1] == b"\n" and t.strip(b"\n") for t in short) and any(t and not t.strip(b"\n") for t in short)
        assert any(t and b"\n" not in t for t in short) and any(t[-1:] == b"\n" for t in long) and any(t[-1:] != b"\n" for t in long)
        assert any(b"\r\n" in t for t in short) and any(b"\r\n" in t for t in long)
        # the last byte of an index block and the first of the next, the last byte of a wavefront's last lane; a window of newlines
        # whatever the misalignment (31 in a row); every one of those newlines ends a retained line or starts one
        ends = set()
        for t in long:
            nl = set(_newlines(t).tolist())
            ends |= {o for o in (1023, 1024, 4095, 4096, 8191, 8192) if o in nl}
        assert ends == {1023, 1024, 4095, 4096, 8191, 8192}
        assert any(b"\n" * 31 in t for t in long) and any(b"\n" * 16 in t for t in short)
        # a missed or an invented newline changes the answer: retained lines on both sides, or the line number of an error
        kinds = {bool(sc.expected(t, sc.IDX, paf=paf).error) for t in long}
        assert kinds == {False, True}
        assert all(len(sc.expected(t, sc.IDX, paf=paf).recs) > 150 for t in long[:2])


def test_field_alignment_starts_and_ends_every_field_on_every_residue():
    cases = dict(sc.field_alignment())
    text = cases["every residue"]
    assert sc.field_spans(text) == {(k, b, e) for k in range(1, 13) for b in range(8) for e in range(8)}
    want = sc.expected(text, sc.IDX)
    assert want.error is None and len(want.recs) == 64  # every line is retained
    # field lengths 1 to 17, every separator alone and in a run, white space in front and behind
    lines = text.split(b"\n")[:-1]
    assert {len(f) for ln in lines for f in ln.decode().split()[:12]} >= set(range(1, 18))
    for s in sc.SEPS.encode():
        one = bytes([s])
        assert any(one in ln.strip(sc.SEPS.encode()) for ln in lines)
    white = set(sc.SEPS.encode())
    runs = {ln[i] for ln in lines for i in range(1, len(ln)) if ln[i] in white and ln[i - 1] in white}
    assert len(runs) >= 5 and any(ln[0] in white for ln in lines) and any(ln[-1] in white for ln in lines)
    # odd bytes inside QNAME, QUAL and tag values; a low byte directly before and directly after a separator
    low = set(sc.LOW)
    for k in (0, 10):
        col = b"".join(ln.decode().split()[k].encode() for ln in lines)
        assert set(col) & low and sc.E_ACUTE in col
    tags = b"".join(f.encode() for ln in lines for f in ln.decode().split()[12:])
    assert set(tags) & low and sc.E_ACUTE in tags
    assert set(bytes(range(1, 9)) + bytes(range(0x0e, 0x1c))) <= set(text)
    edge = cases["low bytes around a separator"]
    assert b"\x01\t" in edge and b"\t\x02" in edge and len(sc.expected(edge, sc.IDX).recs) == 3
    # side arrays worth comparing: placed and unplaced, piled and not, NM in the twelfth field and behind others
    assert 20 < int((want.places["span"] > 0).sum()) < 64 and int((want.bases[0]["span"] > 0).sum()) > 20
    assert int((want.edits["nm"] != 0xFFFFFFFF).sum()) == 64


def test_field_counts_hold_every_count_and_every_error():
    cases = sc.field_counts()
    assert len({n for n, _ in cases}) == len(cases)
    wants = {name: sc.expected(text, sc.IDX) for name, text in cases}
    counts = {}
    for name, text in cases:
        for ln in sc.split_lines(text):
            if ln.startswith("@") or len(text) > (1 << 20):
                continue
            f = ln.strip().split()
            form = "short" if len(f) < 6 else "star" if f[5] == "*" else "flag4" if f[1].isdigit() and int(f[1]) & 4 else "retained"
            counts.setdefault(len(f), set()).add(form)
    for nf in range(6):
        assert "short" in counts[nf]
    for nf in range(6, 14):
        assert counts[nf] >= {"star", "flag4", "retained"}, nf
    # every error kind alone, and every pair that one line can hold: the definition's order
    for kinds in sc.error_sets():
        got = wants["raises: " + " and ".join(kinds)].error
        assert got is not None and got[0] is sc.ERROR_TYPE[kinds[0]] and got[2] == 2, kinds
    assert len(sc.error_sets()) == 7 + 19
    for nf in range(6, 12):
        assert wants["retained line of %d fields" % nf].error[0] is IndexError
    assert {w.error[2] for n, w in wants.items() if " at line 300, " in n} == {300}
    assert {w.error[0] for w in wants.values() if w.error} == set(sc.KIND_OF)
    # header lines; ' @x' is no header line
    assert wants["0 to 13 fields that raise nothing, header lines"].qnames == ["n12r", "n13r", "@x"]
    # numbers
    assert [int(r["flag_len"]) & 0xFFF for r in wants["FLAG forms"].recs][:4] == [16, 0xFF8, 0, 16] and len(wants["FLAG forms"].recs) == 5
    assert wants["NM forms that parse"].edits["nm"].tolist() == [3, 0, 0xFFFFFFFF, 7, 9]
    c = wants["CIGAR forms"].recs
    assert len(c) == 10 and c["total"][6] == c["matched"][6] == 0xFFFFFFFF and c["total"][7] == c["total"][8] == 0xFFFFFFFF
    assert int(c["matched"][0]) == 1 + 12 % 3 and int(c["matched"][1]) == 0
    assert (wants["SEQ * and of one base"].recs["flag_len"] >> 12).tolist() == [0, 1]
    assert int(wants["SEQ of the longest length"].recs["flag_len"][1]) >> 12 == sc.MAX_SEQLEN
    assert wants["SEQ one longer than that"].error[0] is OverflowError
    assert sum(len(t) > (1 << 20) for _, t in cases) == 2  # the only multi-megabyte lines


def test_qnames_hold_every_length_and_relation():
    cases = sc.qnames()
    got = set()
    for name, text in cases:
        want = sc.expected(text, sc.IDX)
        assert want.error is None
        got |= sc.relations(want.qnames)
        # lines that are not retained, with names of their own, between two equal names: no new read
        lines = sc.split_lines(text)
        kept = [i for i, ln in enumerate(lines) if cv.retained_fields(ln) is not None]
        gaps = [(a, b) for a, b in zip(kept, kept[1:]) if b - a > 1]
        assert gaps and all(lines[a].split()[0] == lines[b].split()[0] for a, b in gaps)
        assert all(not (want.recs["ref_new"][kept.index(b)] >> 31) for _, b in gaps)
        prevs = sc.prev_qnames(text)
        q = want.qnames[0]
        assert prevs[0] == "" and prevs[1] == q and prevs[2] == q[:-1] and prevs[3][:-1] == q and len(prevs[4]) == 300 and prevs[4] != q
        assert [bool(sc.expected(text, sc.IDX, p).recs["ref_new"][0] >> 31) for p in prevs] == [True, False, True, True, True]
    for n in sc.QNAME_LENGTHS:
        for rel in ("equal", "first byte", "last byte", "prefix first", "prefix second"):
            assert (rel, n) in got, (rel, n)
    assert sc.QNAME_LENGTHS == [1, 15, 16, 17, 254, 255, 300]


def test_many_lines_cross_the_grid():
    ncu = 2  # (the GPU test reads the device's count; the table's shape does not depend on it)
    text, where = sc.many_lines(ncu)
    grid = sc.grid_lines(ncu)
    lines = text.split(b"\n")
    n = len(lines) - 1
    assert grid == 256 * 16 * ncu and n == grid + 100000 and lines[-1] == b""
    assert {0, n - 1, grid - 1, grid} <= set(where) and max(len(ln) for i, ln in enumerate(lines) if i not in set(where)) == 1
    assert len(text) < 1.6 * n
    want = sc.expected(text, sc.IDX)
    assert len(want.recs) == len(where)
    k = where.index(grid)
    assert want.qnames[k - 1] == want.qnames[k] == "edge" and not want.recs["ref_new"][k] >> 31 and want.recs["ref_new"][k - 1] >> 31
    assert 0 < int((want.recs["ref_new"] >> 31).sum()) < len(where)


def test_paf_fields_hold_what_they_list():
    cases = dict(sc.paf_fields())
    wants = {name: sc.expected(text, sc.IDX, paf=True) for name, text in cases.items()}
    good = wants["lines that raise nothing"]
    assert good.error is None and "f11" not in good.qnames and {"f12", "f13", "", "read 1", "back", "neg"} <= set(good.qnames)
    assert wants["CRLF"].error is None and np.array_equal(wants["CRLF"].recs, good.recs[:len(wants["CRLF"].recs)])
    flags = {q: int(r["flag_len"]) & 0xFFF for q, r in zip(good.qnames, good.recs)}
    assert flags["minus"] == 16 | 256 and flags["ss"] == 256 and flags["tabs"] == 256  # (the second 'ss' line: tp:AxS)
    by = {}
    for q, r in zip(good.qnames, good.recs):
        by.setdefault(q, []).append(r)
    assert [int(r["flag_len"]) & 256 for r in by["twice"]] == [0, 256] and [int(r["flag_len"]) & 256 for r in by["five"]] == [256, 0]
    assert [int(r["flag_len"]) & 256 for r in by["ss"]] == [0, 256]
    assert (int(by["five"][1]["matched"]), int(by["five"][1]["total"])) == (9, 9)
    assert (int(by["cg"][0]["matched"]), int(by["cg"][0]["total"])) == (5, 22 + 5) and (int(by["cg"][1]["matched"]), int(by["cg"][1]["total"])) == (6, 10)
    assert int(by["back"][0]["total"]) == 10 + 30 and int(by["neg"][0]["total"]) == 10 + 10
    kinds = {name: w.error[0] for name, w in wants.items() if w.error}
    assert kinds["raises: zero total"] is ZeroDivisionError and kinds["raises: unknown target"] is KeyError
    assert kinds["raises: zero total and unknown target"] is ZeroDivisionError and kinds["raises: no number and zero total"] is ValueError
    assert kinds["raises: negative length"] is OverflowError and kinds["raises: negative matches"] is OverflowError
    assert set(kinds.values()) == {ZeroDivisionError, KeyError, ValueError, OverflowError}


def test_expected_is_the_host_tokeniser_plus_the_splitting_rule():
    dbtext, accs, taxids = samgen.make_dbinfo(seed=8, n_species=12)
    idx = {"Unmapped": 0}
    idx.update({a: i + 1 for i, a in enumerate(accs)})
    for text in (samgen.make_sam_single(3, 800, accs, taxids), samgen.make_sam_paired(4, 500, accs, taxids)):
        want = mp.tokenise_sam(text.splitlines(True), idx)
        got = sc.expected(text.encode(), idx)
        assert got.error is None and np.array_equal(got.recs, want) and len(want) > 300
        assert np.array_equal(sc.expected(text.encode().rstrip(b"\n"), idx).recs, want)  # a trailing unterminated line is a line
    # only b"\n" ends a line: the bytes str.splitlines() would also cut at stay inside their line (and, white space, split its fields)
    ln = sc.sam_line("q", tags=("NM:i:1", "XA:Z:a\x0bb\x0cc\x1cd\x1de\x1ef")).decode()
    assert len(ln.splitlines()) > 1 and sc.split_lines(ln.encode() + b"\n") == [ln]
    assert len(sc.expected((ln + "\n").encode(), sc.IDX).recs) == 1
    assert sc.split_lines(b"") == [] and sc.split_lines(b"\n") == [""] and sc.split_lines(b"a\n\nb") == ["a", "", "b"]
    assert sc.split_lines(b"a\r\n") == ["a\r"]
    # an error is the first raising line's, with the definition's own message
    e = sc.expected(b"x\n" + sc.error_line("b", ("key",)) + b"\n" + sc.error_line("c", ("flag",)) + b"\n", sc.IDX).error
    assert e == (KeyError, "'NOPE.1'", 1)


@pytest.mark.parametrize("name,line", sc.DEPARTURES)
def test_known_departures_are_what_the_definition_accepts(name, line):
    """DESIGN.md §4, "Known departures of the text tokeniser": the definition takes each of these lines as a retained line (the
    device parser, byte by byte, cannot), and none of them is in a family."""
    want = sc.expected(line, sc.IDX)
    assert want.error is None and len(want.recs) == 1, name
    text = line.decode("utf-8")
    f = text.strip().split()
    assert len(f) == 12
    if "underscore" in name:
        assert "_" in f[1] + f[11] and int(f[1]) in (0, 16) and int(f[11][5:]) in (0, 10)
    elif "separator" in name:
        assert len(sc.ascii_fields(line)) == 11  # (what the device sees)
    else:
        assert not f[5].isascii() and int(want.recs["total"][0]) == 5


def test_no_family_holds_a_departure():
    for fam in (sc.window_edges, sc.field_alignment, sc.field_counts, sc.qnames, sc.paf_fields):
        for _, t in fam():
            if len(t) > (1 << 20):
                continue
            for ln in sc.split_lines(t):
                f = ln.split()
                assert f == [x.decode() for x in sc.ascii_fields(ln.encode())]  # no non-ASCII separator
                if fam is not sc.paf_fields and len(f) >= 6 and not ln.startswith("@"):
                    assert "_" not in f[1] and f[5].isascii() and (len(f) < 12 or "_" not in f[11])
