"""--coverage on the host: the definition (metalign_amd/coverage.py) against hand tables and a per-base array, the placement
arithmetic of mg_coverage_core.h compiled with g++ against the definition, the flag and map_main's refusals."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import bamgen
import coverage_cases as cc
from metalign_amd import cli
from metalign_amd import coverage as cv

HERE = os.path.dirname(os.path.abspath(__file__))

# acc -> [length, taxid, names, lineage]: two genomes, g1 of three contigs (one never hit), g2 of one
A2I = {"Unmapped": [0, "Unmapped", "", ""], "c1": [1000, "g1.1", "", ""], "c2": [1000, "g1.1", "", ""], "c3": [1000, "g1.1", "", ""],
       "d1": [500, "g2", "", ""]}
T2I = {"Unmapped": [0], "g1.1": [3000], "g2": [500]}
HEAD = ["@HD\tVN:1.6\n", "@SQ\tSN:c1\tLN:200\n", "@SQ\tSN:c2\tLN:7\n", "@SQ\tSN:c2\tLN:300\n", "@SQ\tSN:zz\tLN:9\n", "@SQ\tLN:5\n",
        "@SQ\tSN:c3\n", "@PG\tID:x\n"]


def L(q, flag, rname, pos, cigar, seq="ACGT", tag="NM:i:0"):
    return "\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "*", tag]) + "\n"


def test_lengths_sq_overrides_dbinfo_last_wins_missing_falls_back():
    # (the alignment line ends the leading header block: the @SQ line behind it is no header line)
    got = cv.coverage(HEAD + [L("r", 0, "c1", 1, "4M"), "@SQ\tSN:d1\tLN:1\n"], A2I, 0.5)
    assert got.lengths == {"Unmapped": 0, "c1": 200, "c2": 300, "c3": 1000, "d1": 500}
    assert cv.sq_length("@SQ\tSN:a\tLN:12x\n") is None and cv.sq_length(b"@SQ\tLN:12\tSN:a\r\n") == ("a", 12)


def test_hand_table():
    lines = HEAD + [
        L("a", 0, "c1", 1, "10M"),                  # [0, 10)
        L("a", 256, "c1", 6, "10M", seq="*"),       # a secondary counts: [5, 15)
        L("b", 16, "c1", 196, "10M"),               # clipped at 200: [195, 200)
        L("b2", 0, "c1", 200, "3M"),                # pos0 = L - 1: [199, 200)
        L("c", 0, "c1", 201, "10M"),                # pos0 = L: unplaced
        L("d", 0, "c1", 0, "10M"),                  # POS 0: unplaced
        L("d2", 0, "c1", "x7", "10M"),              # not a number: unplaced, no error
        L("d3", 0, "c1", "12345678901", "10M"),     # 11 digits: unplaced
        L("d4", 0, "c1", str(2 ** 31), "10M"),      # above 2^31 - 1: unplaced
        L("e", 0, "c1", 50, "10S30I"),              # fails pct_id 0.5: does not count at all
        L("f", 2048, "c1", 100, "10M"),             # supplementary: does not count
        L("g", 0, "c1", 100, "5M5S"),               # matched / total == 0.5 exactly: counts, [99, 104)
        L("h", 0, "c1", 120, "4M6S"),               # 0.4: does not count
        L("i", 4, "c1", 1, "10M"),                  # unmapped: not retained
        L("j", 0, "c1", 1, "*"),                    # not retained
        L("k", 0, "c2", 10, "10M5D10M2X3N1I"),      # D, N and X count, one block: [9, 39)
        L("l", 0, "d1", 491, "20M"),                # db_info's length (no @SQ): [490, 500)
        b"m\t0\td1\t1\t60\t8M\t*\t0\t0\tACGT\t*\tNM:i:0\n",  # bytes
    ]
    got = cv.coverage(lines, A2I, 0.5)
    assert got.unplaced == 5
    assert got.per == {"c1": [5, 10 + 10 + 5 + 1 + 5, 15 + 5 + 5], "c2": [1, 30, 30], "d1": [2, 18, 18]}
    # at pct_id 0 the soft-clipped insertion counts, and has no reference base: one more unplaced
    got0 = cv.coverage(lines, A2I, 0.0)
    assert got0.unplaced == 6 and got0.per["c1"][0] == 6
    rows = cv.rows(got, A2I, T2I)
    assert rows == [("S", "c1", "g1.1", 200, 5, 31, 25), ("S", "c2", "g1.1", 300, 1, 30, 30), ("S", "d1", "g2", 500, 2, 18, 18),
                    ("G", "g1.1", "g1.1", 200 + 300 + 1000, 6, 61, 55), ("G", "g2", "g2", 500, 2, 18, 18)]


def test_a_line_stage_c_would_drop_is_counted():
    # the file's first read loses its first line in stage C (the phantom boundary); coverage sees both lines
    got = cv.coverage([L("first", 0, "d1", 1, "10M"), L("first", 256, "d1", 101, "10M", seq="*")], A2I, 0.5)
    assert got.per == {"d1": [2, 20, 20]}


def test_lines_the_tokeniser_raises_on_still_raise():
    for line, exc in ((L("a", 0, "nope", 1, "4M"), KeyError), (L("a", 0, "c1", 1, "4="), ValueError),
                      ("a\t0\tc1\t1\t60\t4M\t*\t0\t0\tACGT\t*\n", IndexError), (L("a", 0, "c1", 1, "M"), ZeroDivisionError),
                      (L("a", "x", "c1", 1, "4M"), ValueError), (L("a", 0, "c1", 1, "4M", tag="NM:i:x"), ValueError)):
        with pytest.raises(exc):
            cv.coverage([line], A2I, 0.5)


def test_exact_bytes_of_the_tsv_two_files(tmp_path):
    got = cv.coverage(HEAD + [L("a", 0, "c1", 1, "10M"), L("b", 0, "c1", 6, "10M"), L("c", 0, "c1", 0, "1M")], A2I, 0.5)
    path = str(tmp_path / "cov.tsv")
    cv.write_coverage(path)
    cv.write_coverage(path, cv.rows(got, A2I, T2I), got.unplaced, source="one.sam", append=True)
    cv.write_coverage(path, [], 0, source="two.bam", append=True)
    want = ("#kind\tid\ttaxid\tlength\talignments\taligned_bases\tcovered_bases\tbreadth\tmean_depth\texpected_breadth\n"
            "#file\tone.sam\n"
            "S\tc1\tg1.1\t200\t2\t20\t15\t0.075000\t0.100000\t0.095163\n"
            "G\tg1.1\tg1.1\t1500\t2\t20\t15\t0.010000\t0.013333\t0.013245\n"
            "#unplaced\t1\n"
            "#file\ttwo.bam\n"
            "#unplaced\t0\n")
    assert open(path).read() == want
    cv.write_coverage(path, cv.rows(got, A2I, T2I), got.unplaced)  # one input file: no #file line
    assert open(path).read() == want.split("#file\tone.sam\n")[0] + want.split("#file\tone.sam\n")[1].split("#file")[0]


def _brute(placed, lengths):
    per, unplaced = {}, 0
    arrays = {}
    for acc, pos0, span in placed:
        Ln = lengths[acc]
        if span == 0 or pos0 >= Ln:
            unplaced += 1
            continue
        a = arrays.setdefault(acc, np.zeros(Ln, dtype=np.uint32))
        a[pos0:min(pos0 + span, Ln)] += 1
    for acc, a in arrays.items():
        n = sum(1 for p in placed if p[0] == acc and p[2] and p[1] < lengths[acc])
        per[acc] = [n, int(a.sum()), int(np.count_nonzero(a))]
    return per, unplaced


@pytest.mark.parametrize("seed", range(6))
def test_interval_merge_against_a_per_base_array(seed):
    rng = random.Random(seed)
    lengths = {"a%d" % i: rng.choice([0, 1, 2, 31, 32, 33, rng.randrange(1, 5001)]) for i in range(8)}
    placed = []
    for _ in range(rng.randrange(1, 400)):
        acc = rng.choice(list(lengths))
        Ln = lengths[acc]
        placed.append((acc, rng.randrange(0, Ln + 40), rng.choice([0, 1, 2, 31, 32, 33, 64, rng.randrange(1, 700)])))
    # touching and nested intervals and exact duplicates
    placed += [("a7", 10, 5), ("a7", 15, 5), ("a7", 11, 2), ("a7", 10, 5)]
    assert cv.accumulate(placed, lengths) == _brute(placed, lengths)


def test_the_flag_exists_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        act = [a for a in cli.parser_for(tool)._actions if a.dest == "coverage"][0]
        assert act.default == "NONE" and act.option_strings == ["--coverage"]


def test_map_main_refuses_two_processes_and_paf(monkeypatch, tmp_path):
    import stage_c_checks as sc
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    cov = tmp_path / "cov.tsv"
    args = sc.make_args(str(tmp_path / "x.paf"), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"),
                        {"input_type": "AUTO", "coverage": str(cov)})
    with pytest.raises(SystemExit) as e:
        mp.map_main(args)
    assert "PAF" in str(e.value.code) and "\n" not in str(e.value.code) and not cov.exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = sc.make_args(str(tmp_path / "x.sam"), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), {"coverage": str(cov)})
    with pytest.raises(SystemExit) as e:
        mp.map_main(args)
    assert str(e.value.code) == "Error: --coverage runs in one process on one GPU; start it without torch.distributed.run."
    assert not cov.exists()


# ---- mg_coverage_core.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("coverage") / "host_coverage_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-Wall", "-o", out, os.path.join(HERE, "host_coverage_check.cpp")])
    return out


def _run(exe, tmp_path, lines=(), bam=(), intervals=(), clips=(), counts=()):
    blob = struct.pack("<I", len(lines)) + b"".join(struct.pack("<I", len(x)) + x for x in lines)
    blob += struct.pack("<I", len(bam)) + b"".join(struct.pack("<I", len(x)) + x for x in bam)
    blob += struct.pack("<I", len(intervals)) + b"".join(struct.pack("<QQ", b, e) for b, e in intervals)
    blob += struct.pack("<I", len(clips)) + b"".join(struct.pack("<IIQ", *c) for c in clips)
    blob += struct.pack("<I", len(counts)) + b"".join(struct.pack("<IIId", *c) for c in counts)
    p = tmp_path / "in.bin"
    p.write_bytes(blob)
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    return [ln.split() for ln in out.stdout.decode().splitlines()]


def test_core_header_places_lines_and_bam_records_as_the_definition(exe, tmp_path):
    lines = [ln for ln in cc.case(300, 150)[5] if cv.retained_fields(ln) is not None]
    hand = [L("a", 0, "c1", p, c) for p, c in (("x7", "4M"), ("12345678901", "4M"), (str(2 ** 31), "4M"), (str(2 ** 31 - 1), "4M"),
                                                ("0", "4M"), ("007", "4M"), ("5", "4I"), ("5", "3m4M"), ("5", "4294967295M1D"))]
    hand += ["  lead\t0 c1 \x1c 9 \x0b60\x1f5M2D\t*\t0\t0\tAC\t*\tNM:i:0  \n"]  # every white space of str.split()
    assert len(lines) > 500
    want = [cv.placement(cv.retained_fields(ln)) for ln in lines + hand]
    assert len({w for w in want}) > 300 and (0, 0) in want and want[-2] == (4, 2 ** 32 - 1) and want[-1] == (8, 7)
    # (the records bamgen can encode: POS an integer below 2^31)
    as_bam = [ln for ln in lines + hand[4:7]]
    recs = [bamgen.record(ln.rstrip("\n").split("\t"), 0, -1) for ln in as_bam]
    out = _run(exe, tmp_path, lines=[ln.rstrip("\n").encode() for ln in lines + hand], bam=recs)
    got_l = [(int(r[1]), int(r[2])) for r in out if r[0] == "L"]
    got_b = [(int(r[1]), int(r[2])) for r in out if r[0] == "B"]
    assert got_l == want
    assert got_b == [cv.placement(cv.retained_fields(ln)) for ln in as_bam]


def test_core_header_interval_words_clips_and_the_counting_rule(exe, tmp_path):
    edges = [0, 31, 32, 63, 64]
    intervals = [(b, e) for b in edges for e in [x + 1 for x in edges] + edges[1:] if e > b] + [(2 ** 33 + 5, 2 ** 33 + 70)]
    clips = [(0, 0, 10), (0, 5, 10), (9, 5, 10), (10, 5, 10), (5, 5, 10), (0, 1, 0), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 33), (3, 2 ** 32 - 1, 2 ** 40)]
    counts = [(5, 10, 0, 0.5), (4, 10, 0, 0.5), (5, 10, 2048, 0.5), (5, 10, 256 | (40 << 12), 0.5), (0, 40, 0, 0.0), (1, 3, 0, 1 / 3),
              (1, 3, 0, 0.3333333333333334), (95, 100, 16, 0.95)]
    out = _run(exe, tmp_path, intervals=intervals, clips=clips, counts=counts)
    got_i = [tuple(int(x) for x in r[1:]) for r in out if r[0] == "I"]
    got_w = [[int(x) for x in r[1:]] for r in out if r[0] == "W"]
    for (b, e), (w0, m0, w1, m1), masks in zip(intervals, got_i, got_w):
        bits = [sum(1 << (p - 32 * w) for p in range(max(b, 32 * w), min(e, 32 * w + 32))) for w in range(b // 32, (e - 1) // 32 + 1)]
        assert (w0, w1) == (b // 32, (e - 1) // 32)
        assert m0 & m1 == bits[0] if w0 == w1 else (m0 == bits[0] and m1 == bits[-1])
        assert masks == bits[:4], (b, e)
    assert [int(r[1]) for r in out if r[0] == "C"] == [min(p + s, Ln) - p if s and p < Ln else 0 for p, s, Ln in clips]
    assert [int(r[1]) for r in out if r[0] == "K"] == [int(cv.counts(f & 0xFFF, m, t, pct)) for m, t, f, pct in counts]
    assert [int(r[1]) for r in out if r[0] == "K"][:4] == [1, 0, 0, 1]
