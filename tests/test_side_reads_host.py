"""--side_reads unique on the host: the definition (metalign_amd/side_reads.py) against hand-written streams that take every branch
of the read loop's verdict, its consistency with read_assignments, the record-level statement of the rule against the line-level
one, mg_sidemask_core.h under the sanitizers, the flag, its refusal, the memory estimate and the header line."""
import os
import struct
import subprocess

import numpy as np
import pytest

import identity_cases as ic
import side_reads_cases as src
import stage_c_checks as sc
from metalign_amd import _hip, assignments, cli
from metalign_amd import coverage as cv
from metalign_amd import depth as dp
from metalign_amd import identity as idn
from metalign_amd import map_and_profile as mp
from metalign_amd import side_outputs as so
from metalign_amd import side_reads as sr

HERE = os.path.dirname(os.path.abspath(__file__))
A2I, T2I, L = ic.A2I, ic.T2I, ic.L  # c1 c2 c3 -> g1.1, d1 -> g2
NM = ["NM:i:1"]


def _hand():
    """-> (lines, the verdict of every read, the names of the lines that survive).  Single-end reads first, then paired ones: what
    a read is told about pairing are the flags of the NEXT read's first line."""
    named = {}

    def ln(name, q, flag, rname, cigar="10M", raw=False):
        named[name] = L(q, flag, rname, cigar, NM)
        if raw:
            named[name] = named[name].encode()
        return named[name]

    lines = [
        "@HD\tVN:1.6\n", "@SQ\tSN:c1\tLN:1000\n",
        # the file's first read loses its first line to the phantom boundary; its second line makes it unique
        ln("z1", "z", 0, "c1"), ln("z2", "z", 256, "c2"),
        ln("a1", "a", 0, "d1", raw=True),                                # a single-end unique read (a bytes line)
        L("un", 4, "c1", "10M", NM),                                      # unmapped: not retained
        ln("m1", "m", 0, "c1"), ln("m2", "m", 256, "d1"),                # single-end, two lines: multimapped
        ln("s1", "s", 0, "c1"), ln("s2", "s", 2048, "c1"),               # ... a 2048 line still counts as a line: multimapped
        ln("n1", "n", 0, "c1", "4M6S"),                                   # nothing passes pct_id: ambiguous
        ln("x1", "x", 0, "c1"), ln("x2", "x", 256, "c2"),                # after an ambiguous read: x1 is dropped, x2 makes it unique
        ln("q1", "q", 0, "c1", "4M6S"),                                   # ambiguous
        ln("y1", "y", 0, "d1"),                                           # its only line is the dropped one: ambiguous again
        ln("w1", "w", 0, "c1"), ln("w2", "w", 256, "d1"),                # w1 dropped; closed by a paired line, one end: unique (g2)
        # one taxon in `both`, but kept[0] is what is reported: g2, so the d1 line survives and the g1.1 lines do not
        ln("p1", "p", 65, "d1"), ln("p2", "p", 321, "c1"), ln("p3", "p", 129, "c2"),
        # unique for g1.1 with lines on three of its accessions, and one on another taxon
        ln("r1", "r", 65, "c1"), ln("r2", "r", 321, "c3"), ln("r3", "r", 129, "c2"), ln("r4", "r", 385, "d1"),
        # a 2048 line and a line below pct_id inside a unique read: they survive here, the families' own rule refuses them
        ln("u1", "u", 65, "c1"), ln("u2", "u", 2113, "c1"), ln("u3", "u", 129, "c2", "4M6S"), ln("u4", "u", 129, "c2"),
        ln("pm1", "pm", 65, "c1"), ln("pm2", "pm", 321, "d1"), ln("pm3", "pm", 129, "c2"), ln("pm4", "pm", 385, "d1"),  # paired M
        ln("pa1", "pa", 65, "c1"), ln("pa2", "pa", 129, "d1"),           # the ends share no taxon: ambiguous
        ln("t1", "t", 65, "c1"), ln("t2", "t", 129, "c2"),               # t1 dropped, one end left: unique
        ln("pe1", "pe", 65, "c1"), ln("pe2", "pe", 321, "c2"),           # two lines of one end, none of the other: ambiguous
        ln("l1", "l", 65, "c1"), ln("l2", "l", 129, "c1"),               # l1 dropped; the last read is never decided
    ]
    verdicts = [("z", "U", ["g1.1"]), ("a", "U", ["g2"]), ("m", "M", ["g1.1", "g2"]), ("s", "M", ["g1.1"]), ("n", "A", []),
                ("x", "U", ["g1.1"]), ("q", "A", []), ("y", "A", []), ("w", "U", ["g2"]), ("p", "U", ["g2"]), ("r", "U", ["g1.1"]),
                ("u", "U", ["g1.1"]), ("pm", "M", ["g1.1", "g2", "g1.1", "g2"]), ("pa", "A", []), ("t", "U", ["g1.1"]), ("pe", "A", []),
                ("l", "N", [])]
    survive = ["z2", "a1", "x2", "w2", "p1", "r1", "r2", "r3", "u1", "u2", "u3", "u4", "t2"]
    return lines, verdicts, named, survive


def test_hand_streams_take_every_branch():
    lines, verdicts, named, survive = _hand()
    assert [r[:3] for r in assignments.read_assignments(lines, A2I, 0.5)] == verdicts
    got = list(sr.unique_lines(lines, A2I, 0.5))
    assert got[:2] == lines[:2]  # the header lines, unchanged and first
    assert [id(x) for x in got[2:]] == [id(named[k]) for k in survive]  # (the same objects, bytes or str, in file order)
    # the families then apply their own rule: u2 (2048) and u3 (below pct_id) do not count
    cov = cv.coverage(sr.unique_lines(lines, A2I, 0.5), A2I, 0.5)
    assert {a: v[0] for a, v in cov.per.items()} == {"c1": 2, "c2": 5, "c3": 1, "d1": 3}
    assert {a: v[0] for a, v in cv.coverage(lines, A2I, 0.5).per.items()} == {"c1": 14, "c2": 8, "c3": 1, "d1": 9}
    ident = idn.identity(sr.unique_lines(lines, A2I, 0.5), A2I, 0.5)
    assert sum(v[0] for v in ident.per.values()) + ident.unscored == 11
    dep = dp.depth(sr.unique_lines(lines, A2I, 0.5), A2I, 0.5, 0)
    assert {a: v[0] for a, v in dep.per.items()} == {"c1": 2, "c2": 5, "c3": 1, "d1": 3}


def test_a_stream_of_header_lines_only_and_an_empty_one():
    assert list(sr.unique_lines(["@HD\tVN:1.6\n", b"@SQ\tSN:c1\tLN:5\n"], A2I, 0.5)) == ["@HD\tVN:1.6\n", b"@SQ\tSN:c1\tLN:5\n"]
    assert list(sr.unique_lines([], A2I, 0.5)) == []
    one = [L("only", 0, "c1", "10M", NM), "@CO\tlate\n"]
    assert list(sr.unique_lines(one, A2I, 0.5)) == ["@CO\tlate\n"]  # (its only line is the phantom's; the read is 'N' anyway)


# ---- generated streams ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated():
    out = []
    for nsingle, npairs, seed in ((300, 150, 41), (0, 260, 42), (500, 0, 43)):
        _, accs, acc2info, taxid2info, _, lines = ic.case(nsingle, npairs, seed=seed)
        out.append((lines, acc2info, taxid2info))
    return out


def _retained(lines):
    return [ln for ln in lines if assignments._fields_of(ln) is not None]


def test_unique_reads_are_the_profiles_unique_counts(generated):
    for lines, acc2info, _ in generated:
        unique, _, total, _ = assignments.fold(assignments.read_assignments(lines, acc2info, 0.5))
        reads = {}
        for ln in sr.unique_lines(lines, acc2info, 0.5):
            if not ln.startswith("@"):
                f = ln.split()
                reads.setdefault(acc2info[f[2]][1], set()).add(f[0])
        assert total > 100 and len(unique) > 3
        assert {t: len(q) for t, q in reads.items()} == {t: v[0] for t, v in unique.items()}


def _words_of(rows, taxids):
    """read_assignments' rows -> the verdict words of mg_profile_commit_assign_dev (word 1 plays no part in the rule)."""
    tax_index = {t: i for i, t in enumerate(taxids)}
    kind = {"A": 0, "U": 1, "M": 2, "N": 3}
    words = np.zeros(2 * len(rows), dtype=np.uint64)
    for r, (_, cls, tx, hit) in enumerate(rows):
        words[2 * r] = kind[cls] | ((tax_index[tx[0]] << 2) if cls == "U" else 0)
        words[2 * r + 1] = max(hit, 0)
    return words


def _record_case(lines, acc2info, taxid2info):
    """-> (records, words, ref2tax, the line-level rule's mask over the retained lines)"""
    acc_index, taxids, ref2tax = mp.dense_tables(acc2info, taxid2info)
    recs = mp.tokenise_sam(lines, acc_index)
    words = _words_of(list(assignments.read_assignments(lines, acc2info, 0.5)), taxids)
    alive = {id(ln) for ln in sr.unique_lines(lines, acc2info, 0.5)}
    want = np.array([id(ln) in alive for ln in _retained(lines)], dtype=bool)
    assert len(want) == len(recs)
    return recs, words, ref2tax, want


def test_the_record_rule_is_the_line_rule(generated):
    for lines, acc2info, taxid2info in generated:
        recs, words, ref2tax, want = _record_case(lines, acc2info, taxid2info)
        got = sr.unique_mask_of_records(recs, words, ref2tax)
        assert got.dtype == bool and np.array_equal(got, want)
        assert 0.1 * len(want) < want.sum() < 0.9 * len(want)
        assert sr.outside_of_records(recs, words) == 0
    lines, _, _, _ = _hand()
    t2i = dict(T2I, **{"g1.1": [3000, "strain", "", ""], "g2": [500, "strain", "", ""], "Unmapped": [0, "", "", ""]})
    recs, words, ref2tax, want = _record_case(lines, A2I, t2i)
    assert np.array_equal(sr.unique_mask_of_records(recs, words, ref2tax), want) and want.sum() == 13


def test_the_record_rule_at_its_edges():
    new = _hip.NEW_BIT
    recs = np.array([(0 | new, 1, 1, 0), (1, 1, 1, 0), (1 | new, 1, 1, 0), (2, 1, 1, 0), (5, 1, 1, 0), (0 | new, 1, 1, 0), (0, 1, 1, 0)],
                    dtype=_hip.REC_DTYPE)
    words = np.array([1 | (7 << 2), 0, 1 | (8 << 2), 0, 3, 0], dtype=np.uint64)  # U taxon 7, U taxon 8, N
    ref2tax = np.array([7, 8, 8], dtype=np.uint32)
    # read 0: its NEW line dropped, the next on row 1 is another taxon; read 1: NEW line kept, row 2 kept, row 5 >= nref; read 2: N
    assert sr.unique_mask_of_records(recs, words, ref2tax).tolist() == [False, False, True, True, False, False, False]
    assert sr.unique_mask_of_records(recs, words[:4], ref2tax).tolist() == [False, False, True, True, False, False, False]
    assert sr.outside_of_records(recs, words) == 0 and sr.outside_of_records(recs, words[:4]) == 2
    head = recs.copy()
    head["ref_new"][0] = 0  # a first record without NEW: ordinal -1
    assert sr.unique_mask_of_records(head, words, ref2tax).tolist() == [False, False, False, False, False, False, False]
    assert sr.outside_of_records(head, words) == 2
    assert sr.unique_mask_of_records(recs[:0], words, ref2tax).tolist() == []
    assert sr.unique_mask_of_records(recs, words[:0], ref2tax).tolist() == [False] * 7
    assert sr.unique_mask_of_records(recs, words, ref2tax[:0]).tolist() == [False] * 7


# ---- mg_sidemask_core.h on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sidemask") / "host_sidemask_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_sidemask_check.cpp")])
    return out


def _check_on_host(exe, tmp_path, recs, words, ref2tax):
    want = sr.unique_mask_of_records(recs, words, ref2tax)
    p = tmp_path / "case.bin"
    p.write_bytes(struct.pack("<QQII", len(recs), len(words) // 2, len(ref2tax), sr.outside_of_records(recs, words)) + recs.tobytes()
                  + words.tobytes() + ref2tax.tobytes() + want.astype(np.uint8).tobytes())
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.decode().splitlines()[-1] == "%d records, %d kept, 0 differ" % (len(recs), int(want.sum()))


def test_core_header_against_the_record_rule(exe, tmp_path, generated):
    lines, acc2info, taxid2info = generated[0]
    _check_on_host(exe, tmp_path, *_record_case(lines, acc2info, taxid2info)[:3])
    for n, seed in ((0, 1), (1, 2), (4095, 3), (4096, 4), (4097, 5), (3 * 4096 + 17, 6)):
        _check_on_host(exe, tmp_path, *src.synthetic(n, seed))
    _check_on_host(exe, tmp_path, *src.synthetic(9000, 7, nreads_short=1))      # nreads too small
    _check_on_host(exe, tmp_path, *src.synthetic(9000, 8, nreads_short=10 ** 9))  # no read at all
    _check_on_host(exe, tmp_path, *src.synthetic(9000, 9, first_new=False, p_new=0.001))  # records in front of the first NEW one
    recs, words, ref2tax = src.synthetic(5000, 10)
    share = src.reasons(recs, words, ref2tax)  # (the generated inputs are not vacuous)
    assert share["kept"] >= 0.10 and min(share["kind"], share["dropped"], share["taxon"]) >= 0.05 and share["bounds"] > 0.01, share
    _check_on_host(exe, tmp_path, recs, words, ref2tax[:0])                  # every row at or above nref
    _check_on_host(exe, tmp_path, recs, words, ref2tax[:3])


# ---- the flag, its refusal, the estimate, the header line ----------------------------------------------------------------------
def test_the_flag_on_both_tools():
    for tool, argv in (("metalign", ["r.fq", "data"]), ("map_and_profile", ["x.sam", "data"])):
        p = cli.parser_for(tool)
        assert p.parse_args(argv).side_reads == "all"
        assert p.parse_args(argv + ["--side_reads", "unique"]).side_reads == "unique"
        with pytest.raises(SystemExit):
            p.parse_args(argv + ["--side_reads", "some"])


def _never(*a, **k):
    raise AssertionError("refused before the process group, the GPU or the library is touched")


def _args(tmp_path, **extra):
    return sc.make_args(str(tmp_path / "x.sam"), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)


def test_unique_without_a_family_is_refused_last_and_early(monkeypatch, tmp_path):
    from metalign_amd import metalign, select_db
    monkeypatch.setattr(_hip.Hip, "get", _never)
    monkeypatch.setattr(_hip, "load_library", _never)
    monkeypatch.setattr(select_db, "dist_context", _never)
    monkeypatch.setattr(select_db, "select_main", _never)
    monkeypatch.setattr(mp, "get_acc2info", _never)
    text = "Error: --side_reads unique needs one of --coverage, --depth, --depth_windows, --identity."
    for fn, a in ((mp.map_main, _args(tmp_path, side_reads="unique")),
                  (mp.map_main, _args(tmp_path, side_reads="unique", read_assignments=str(tmp_path / "r.tsv"))),
                  (metalign.main, ["r.fq", "data", "--side_reads", "unique"])):
        with pytest.raises(SystemExit) as e:
            fn(a)
        assert e.value.code == text
    with pytest.raises(SystemExit) as e:  # (the refusals before it come first)
        mp.map_main(_args(tmp_path, side_reads="unique", depth_window_size=0))
    assert e.value.code == "Error: --depth_window_size must be at least 1."
    with pytest.raises(SystemExit) as e:  # (... and with a family, the existing ones apply: PAF)
        mp.map_main(_args(tmp_path, side_reads="unique", identity="i.tsv", paf_input=True))
    assert e.value.code == so.IDENTITY.refuse_paf
    so.check_flags(_args(tmp_path, side_reads="all"))
    for flag in ("coverage", "depth", "depth_windows", "identity"):
        so.check_flags(_args(tmp_path, side_reads="unique", **{flag: "f.tsv"}))
    assert not (tmp_path / "o.cami").exists()


@pytest.mark.parametrize("nrec", [0, 1000])
def test_need_bytes_adds_32_per_record_in_unique_mode_only(tmp_path, nrec):
    lengths = {"a": 2 ** 20, "b": 12345}
    for extra in (dict(coverage="c.tsv"), dict(identity="i.tsv"), dict(depth="d.tsv", depth_windows="w.tsv", identity="i.tsv")):
        base = so.SideOutputs.of(_args(tmp_path, **extra), "x.sam")
        same = so.SideOutputs.of(_args(tmp_path, side_reads="all", **extra), "x.sam")
        uniq = so.SideOutputs.of(_args(tmp_path, side_reads="unique", **extra), "x.sam")
        ln = lengths if base.placed else None
        assert (base.reads, same.reads, uniq.reads) == ("all", "all", "unique") and uniq.unique and not base.unique
        assert same.need_bytes(ln, 2, nrec) == base.need_bytes(ln, 2, nrec)
        assert uniq.need_bytes(ln, 2, nrec) == base.need_bytes(ln, 2, nrec) + 32 * nrec
    none = so.SideOutputs.of(_args(tmp_path, side_reads="unique"), "x.sam")
    assert not none and not none.unique and none.need_bytes(None, 2, nrec) == 0


def test_the_reads_line_only_in_unique_mode(tmp_path):
    names = dict(coverage="c.tsv", depth="d.tsv", depth_windows="w.tsv", identity="i.tsv", read_assignments="r.tsv")
    texts = {}
    for mode in ("all", "unique", None):
        d = tmp_path / str(mode)
        d.mkdir()
        extra = {k: str(d / v) for k, v in names.items()}
        if mode:
            extra["side_reads"] = mode
        so.write_headers(_args(tmp_path, **extra))
        texts[mode] = {k: (d / v).read_text() for k, v in names.items()}
    assert texts["all"] == texts[None]
    for k in ("coverage", "depth", "depth_windows", "identity"):
        head = texts["all"][k]
        assert head.count("\n") == 1 and texts["unique"][k] == head + "#reads\tunique\n"
    assert texts["unique"]["read_assignments"] == texts["all"]["read_assignments"]
    d = tmp_path / "one"
    d.mkdir()
    so.write_headers(_args(tmp_path, side_reads="unique", depth_windows=str(d / "w.tsv")))
    assert (d / "w.tsv").read_text() == texts["unique"]["depth_windows"] and os.listdir(d) == ["w.tsv"]
