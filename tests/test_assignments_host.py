"""--read_assignments on the host: metalign_amd/assignments.py (the definition) against the reference's golden runs, literal cases
with the expected rows written out, the writer's bytes and the command line."""
import hashlib
import json
import os

import pytest

import stage_c_checks as scc
from metalign_amd import assignments as asg
from metalign_amd import cli
from metalign_amd import map_and_profile as mp


# ---- aggregate = reference ---------------------------------------------------------------------------------------------
def _usable(run):
    return not run.get("map_and_process_raises") and not run["args"].get("low_mem")


def _check_fold(sam_path, dbinfo_path, run, tmp_path):
    ov = run["args"]
    args = scc.make_args(sam_path, dbinfo_path, str(tmp_path / "unused.tsv"), ov)
    acc2info, taxid2info = mp.get_acc2info(args)
    with open(sam_path) as fh:
        rows = list(asg.read_assignments(fh, acc2info, args.pct_id))
    unique, n_unmapped, tot_rds, multimapped = asg.fold(rows)
    want = run["taxids2abs"]
    assert want[0][0] == "Unmapped"
    assert [k for k, _ in want[1:]] == list(unique), "taxon set / order of first unique read differs"
    for taxid, row in want[1:]:
        reads, bases = unique[taxid]
        assert row[0] == reads and type(row[0]) is int, (taxid, row[:2], unique[taxid])
        if ov.get("length_normalize"):
            # the golden value is the float sum of hitlen / genome length over the reads (:233-238): an integer number of
            # bases over the genome length, to ~1e-13 relative for these counts — rounding its product recovers the integer
            assert round(row[1] * taxid2info[taxid][0]) == bases, (taxid, row[:2], unique[taxid])
        else:
            assert row[1] == bases and type(row[1]) is int, (taxid, row[:2], unique[taxid])
    if ov.get("no_quantify_unmapped"):
        assert want[0][1][:2] == [0.0, 0.0]
    else:
        assert want[0][1][0] == float(n_unmapped)
        assert want[0][1][1] == float(n_unmapped) / float(tot_rds)
    if "multimapped" in run:
        assert multimapped == run["multimapped"]
    else:
        assert len(multimapped) == run["multimapped_n"]
        assert hashlib.sha256(json.dumps(multimapped).encode()).hexdigest() == run["multimapped_sha256"]
    return len(rows)


@pytest.mark.parametrize("name,idx,run", [c for c in scc.hand_cases() if _usable(c[2])], ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_fold_equals_reference_hand_case(name, idx, run, tmp_path):
    cdir = os.path.join(scc.GOLDEN, "cases")
    _check_fold(os.path.join(cdir, name + ".sam"), os.path.join(cdir, "dbinfo.txt"), run, tmp_path)


@pytest.mark.parametrize("name", sorted(scc.load_bulk()))
def test_fold_equals_reference_bulk(name, tmp_path):
    spec = scc.load_bulk()[name]
    sam, dbp = scc.materialise_bulk(name, spec, tmp_path)
    checked = 0
    for run in spec["runs"]:
        if _usable(run):
            assert _check_fold(sam, dbp, run, tmp_path) > 0
            checked += 1
    assert checked == len(spec["runs"])


def test_hand_cases_cover_what_the_issue_counts():
    assert sum(1 for c in scc.hand_cases() if _usable(c[2])) >= 20


# ---- literal cases ------------------------------------------------------------------------------------------------------
A2I = {"a1": [1000, "t1", "n", "l"], "b1": [500, "t1", "n", "l"], "a2": [1000, "t2", "n", "l"], "a3": [1000, "t3", "n", "l"]}
SEQ = "ACGTACGTAC"


def L(q, flag, acc, cigar="10M", seq=SEQ):
    qual = "*" if seq == "*" else "I" * len(seq)
    return "\t".join([q, str(flag), acc, "7", "60", cigar, "*", "0", "0", seq, qual, "NM:i:0"]) + "\n"


# every text opens with read `h`, whose first line the phantom boundary takes: it is decided on its second line alone
HEAD = [L("h", 0, "a1"), L("h", 256, "a1", seq="*")]
HEAD_ROW = ("h", "U", ["t1"], 0)
PHEAD = [L("h", 99, "a1"), L("h", 147, "a1")]  # a pair: the mate's line is what is left
PHEAD_ROW = ("h", "U", ["t1"], 10)

LITERAL = {
    # :176 — single end, one line; the last read is never decided
    "single_unique_176": (HEAD + [L("r1", 0, "a2"), L("r2", 0, "a3")],
                          [HEAD_ROW, ("r1", "U", ["t2"], 10), ("r2", "N", [], -1)]),
    # :173 — single end, several lines: every kept line's taxid, duplicates kept, SEQ '*' adds no bases
    "single_multi_173": (HEAD + [L("r1", 0, "a1"), L("r1", 256, "a2", seq="*"), L("r1", 272, "b1", seq="*"), L("r2", 0, "a3")],
                         [HEAD_ROW, ("r1", "M", ["t1", "t2", "t1"], 10), ("r2", "N", [], -1)]),
    # :156 — every line fails pct_id: Ambiguous; r2 then loses its first line and is unique on its secondary alone
    "all_filtered_156_then_unique_by_drop": (
        HEAD + [L("r1", 0, "a1", cigar="2M8S"), L("r2", 0, "a2"), L("r2", 256, "a3", seq="*"), L("r3", 0, "a1")],
        [HEAD_ROW, ("r1", "A", [], -1), ("r2", "U", ["t3"], 0), ("r3", "N", [], -1)]),
    # a read whose only line is dropped is Ambiguous itself (:155), and so drops the next read's first line in turn
    "only_line_dropped_cascade": (
        HEAD + [L("r1", 0, "a1", cigar="2M8S"), L("r2", 0, "a2"), L("r3", 0, "a3"), L("r3", 256, "a1", seq="*"), L("r4", 0, "a2")],
        [HEAD_ROW, ("r1", "A", [], -1), ("r2", "A", [], -1), ("r3", "U", ["t1"], 0), ("r4", "N", [], -1)]),
    # :160 — a pair with one end mapped
    "paired_one_end_160": (PHEAD + [L("p1", 73, "a2"), L("p2", 99, "a3")],
                           [PHEAD_ROW, ("p1", "U", ["t2"], 10), ("p2", "N", [], -1)]),
    # :165 — one end unmapped, the other multimapped
    "paired_one_end_multi_165": (PHEAD + [L("p1", 73, "a2"), L("p1", 329, "a3", seq="*"), L("p2", 99, "a1")],
                                 [PHEAD_ROW, ("p1", "A", [], -1), ("p2", "N", [], -1)]),
    # :165 — both ends mapped, no taxon in common
    "paired_disagree_165": (PHEAD + [L("p1", 99, "a2"), L("p1", 147, "a3"), L("p2", 99, "a1")],
                            [PHEAD_ROW, ("p1", "A", [], -1), ("p2", "N", [], -1)]),
    # :167 — the ends agree on one taxon
    "paired_agree_167": (PHEAD + [L("p1", 99, "a2"), L("p1", 147, "a2"), L("p1", 403, "a3", seq="*"), L("p2", 99, "a1")],
                         [PHEAD_ROW, ("p1", "U", ["t2"], 20), ("p2", "N", [], -1)]),
    # :169 — the ends agree on two taxa: the lines of those taxa, in file order (a1's is left out)
    "paired_multi_169": (PHEAD + [L("p1", 99, "a2"), L("p1", 355, "a3", seq="*"), L("p1", 147, "a2"), L("p1", 403, "a3", seq="*"),
                                  L("p1", 403, "a1", seq="*"), L("p2", 99, "a1")],
                         [PHEAD_ROW, ("p1", "M", ["t2", "t3", "t2", "t3"], 20), ("p2", "N", [], -1)]),
    # the pair flags process_read is told are the NEXT read's (:225-226): a single-end read closed by a paired line
    "single_closed_by_paired_line": (HEAD + [L("r1", 0, "a2"), L("r1", 256, "a3", seq="*"), L("p2", 99, "a1")],
                                     [HEAD_ROW, ("r1", "A", [], -1), ("p2", "N", [], -1)]),
    # a supplementary line is dropped from the list, but a single-end read's line count is not lowered (:137-140)
    "supplementary_single": (HEAD + [L("r1", 0, "a2"), L("r1", 2048, "a3", cigar="5M5H", seq="ACGTA"), L("r2", 0, "a1")],
                             [HEAD_ROW, ("r1", "M", ["t2"], 15), ("r2", "N", [], -1)]),
    # '@', short, flag-4 and '*'-CIGAR lines neither open nor close a read
    "noise_lines": (["@HD\tVN:1.6\n"] + HEAD + [L("x", 4, "*", cigar="*"), "short line\n", L("y", 0, "a2", cigar="*"),
                                                L("h", 256, "a2", seq="*"), "@CO\tmid\n", L("r1", 0, "a3"), L("r2", 0, "a1")],
                    [("h", "M", ["t1", "t2"], 0), ("r1", "U", ["t3"], 10), ("r2", "N", [], -1)]),
    # a QNAME that comes back later is a new read
    "qname_reappears": (HEAD + [L("r1", 0, "a2"), L("h", 0, "a3"), L("r1", 0, "a1")],
                        [HEAD_ROW, ("r1", "U", ["t2"], 10), ("h", "U", ["t3"], 10), ("r1", "N", [], -1)]),
    "one_read": ([L("r0", 0, "a1")], [("r0", "N", [], -1)]),
    "empty": ([], []),
    "header_only": (["@HD\tVN:1.6\n", "@SQ\tSN:a1\tLN:1000\n"], []),
}


@pytest.mark.parametrize("name", sorted(LITERAL))
def test_literal(name):
    lines, want = LITERAL[name]
    assert len(lines) <= 12
    assert list(asg.read_assignments(lines, A2I, 0.5)) == want
    assert list(asg.read_assignments([ln.encode() for ln in lines], A2I, 0.5)) == want  # (a file opened in binary mode)


def test_literal_cases_agree_with_the_loop_they_were_written_from(tmp_path):
    """The same texts through map_and_process's host tokeniser and the CPU oracle, folded: the hand-written rows and the
    package's record-level definition of the reference loop say the same."""
    import oracle
    for name, (lines, want) in sorted(LITERAL.items()):
        if not want:
            continue
        t2i = {"Unmapped": [0, "strain", "n", "l"], "t1": [1500, "strain", "n", "l"], "t2": [1000, "strain", "n", "l"],
               "t3": [1000, "strain", "n", "l"]}
        a2i = dict(A2I)
        args = scc.make_args("-", "-", "-", {})
        t2a, mm, _ = mp.map_and_process(args, lines, a2i, t2i, _assign=oracle.profile_assign)
        unique, n_unmapped, tot, multimapped = asg.fold(want)
        assert {k: v[:2] for k, v in t2a.items() if k != "Unmapped"} == unique, name
        assert [k for k in t2a if k != "Unmapped"] == list(unique), name
        assert t2a["Unmapped"][0] == float(n_unmapped), name
        assert mm == multimapped, name


# ---- the writer --------------------------------------------------------------------------------------------------------
def test_writer_bytes(tmp_path):
    p = tmp_path / "a.tsv"
    rows = [("r1", "U", ["562.1"], 150), ("r 2", "M", ["10", "11", "10"], 72), ("r3", "A", [], -1), ("r4", "N", [], -1)]
    asg.write_assignments(str(p), rows)
    assert p.read_bytes() == (b"#read\tclass\ttaxids\thit_bases\n" b"r1\tU\t562.1\t150\n" b"r 2\tM\t10,11,10\t72\n"
                              b"r3\tA\t-\t-1\n" b"r4\tN\t-\t-1\n")
    asg.write_assignments(str(p), [("r5", "U", ["7"], 1)], append=True)  # (a second input file)
    assert p.read_bytes().endswith(b"r4\tN\t-\t-1\nr5\tU\t7\t1\n") and p.read_bytes().count(b"#read") == 1
    asg.write_assignments(str(p), [])
    assert p.read_bytes() == b"#read\tclass\ttaxids\thit_bases\n"


def test_rows_from_words():
    import numpy as np
    words = np.array([1 | (2 << 2), 40, 0, 0, 2, 0, 3, 0], dtype=np.uint64)
    rows = list(asg.rows_from_words(words, b"r1rr2r3xr4", np.array([0, 2, 5, 7, 10], dtype=np.uint64), ["t0", "t1", "t2"],
                                    np.array([0, 2], dtype=np.uint64), np.array([1, 0], dtype=np.uint32), np.array([9], dtype=np.uint64)))
    assert rows == [("r1", "U", ["t2"], 40), ("rr2", "A", [], -1), ("r3", "M", ["t1", "t0"], 9), ("xr4", "N", [], -1)]
    with pytest.raises(ValueError):
        list(asg.rows_from_words(words, b"", np.array([0], dtype=np.uint64), [], [], [], []))


# ---- the command line --------------------------------------------------------------------------------------------------
def test_flag_on_the_two_parsers_only():
    a = cli.parser_for("map_and_profile").parse_args(["x.sam", "data"])
    assert a.read_assignments == "NONE"
    a = cli.parser_for("map_and_profile").parse_args(["x.sam", "data", "--read_assignments", "out.tsv"])
    assert a.read_assignments == "out.tsv"
    a = cli.parser_for("metalign").parse_args(["r.fq", "data", "--read_assignments", "out.tsv"])
    assert a.read_assignments == "out.tsv"
    with pytest.raises(SystemExit):
        cli.parser_for("select_db").parse_args(["r.fq", "data", "--read_assignments", "out.tsv"])


def test_refused_in_a_multi_gpu_launch(monkeypatch, tmp_path):
    from metalign_amd import select_db

    def no_gpu_work():
        raise AssertionError("the launch is refused before the process group or the GPU is touched")
    monkeypatch.setattr(select_db, "dist_context", no_gpu_work)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    cdir = os.path.join(scc.GOLDEN, "cases")
    out = tmp_path / "abund.tsv"
    args = scc.make_args(os.path.join(cdir, "paired_mix.sam"), os.path.join(cdir, "dbinfo.txt"), str(out),
                         {"read_assignments": str(tmp_path / "reads.tsv")})
    with pytest.raises(SystemExit) as e:
        mp.map_main(args)
    assert "--read_assignments" in str(e.value) and "one process" in str(e.value)
    assert not out.exists() and not (tmp_path / "reads.tsv").exists()
