"""--depth / --depth_windows on the host: the definition (metalign_amd/depth.py) against hand tables and a per-base array, its
invariants with coverage.py, the exact bytes of both files, the device algorithm of mg_depth_core.h run serially under the
sanitizers against the definition, the flags and map_main's refusals."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import depth_cases as dc
from metalign_amd import cli
from metalign_amd import coverage as cv
from metalign_amd import depth as dp

HERE = os.path.dirname(os.path.abspath(__file__))

# (the tables and lines of test_coverage_host.py::test_hand_table)
A2I = {"Unmapped": [0, "Unmapped", "", ""], "c1": [1000, "g1.1", "", ""], "c2": [1000, "g1.1", "", ""], "c3": [1000, "g1.1", "", ""],
       "d1": [500, "g2", "", ""]}
T2I = {"Unmapped": [0], "g1.1": [3000], "g2": [500]}
HEAD = ["@HD\tVN:1.6\n", "@SQ\tSN:c1\tLN:200\n", "@SQ\tSN:c2\tLN:7\n", "@SQ\tSN:c2\tLN:300\n", "@SQ\tSN:zz\tLN:9\n", "@SQ\tLN:5\n",
        "@SQ\tSN:c3\n", "@PG\tID:x\n"]


def L(q, flag, rname, pos, cigar, seq="ACGT", tag="NM:i:0"):
    return "\t".join([q, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", seq, "*", tag]) + "\n"


HAND = HEAD + [
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


def test_hand_table_histograms_statistics_and_windows():
    got = dp.depth(HAND, A2I, 0.5, window=7)
    assert got.unplaced == 5 and got.window == 7
    assert got.lengths == {"Unmapped": 0, "c1": 200, "c2": 300, "c3": 1000, "d1": 500}
    # c1: [0,5) 1, [5,10) 2, [10,15) 1, [99,104) 1, [195,199) 1, [199,200) 2
    assert got.per == {"c1": [5, {0: 175, 1: 19, 2: 6}], "c2": [1, {0: 270, 1: 30}], "d1": [2, {0: 482, 1: 18}]}
    assert got.windows == {"c1": [(0, 9, 7), (1, 10, 7), (2, 1, 1), (14, 5, 5), (27, 1, 1), (28, 5, 4)],
                           "c2": [(1, 5, 5), (2, 7, 7), (3, 7, 7), (4, 7, 7), (5, 4, 4)],
                           "d1": [(0, 7, 7), (1, 1, 1), (70, 7, 7), (71, 3, 3)]}
    rows = dp.rows(got, A2I, T2I)
    # the G row of g1.1 takes c3, never hit, into bin 0
    assert rows == [("S", "c1", "g1.1", 200, {0: 175, 1: 19, 2: 6}), ("S", "c2", "g1.1", 300, {0: 270, 1: 30}),
                    ("S", "d1", "g2", 500, {0: 482, 1: 18}), ("G", "g1.1", "g1.1", 1500, {0: 175 + 270 + 1000, 1: 49, 2: 6}),
                    ("G", "g2", "g2", 500, {0: 482, 1: 18})]
    # c1: ranks 0..174 hold 0, 175..193 hold 1, 194..199 hold 2; t = 10: ranks 10..189 have fifteen 1s among 180
    s = dp.stats(rows[0][4])
    assert s == dp.Stats(200, Fraction(31, 200), 0, Fraction(15, 180), Fraction(19 + 24, 200) - Fraction(31, 200) ** 2, 2, 25, 0, 0, 0)
    assert dp.format_row(rows[0]) == "S\tc1\tg1.1\t200\t0.155000\t0\t0.083333\t0.190975\t2\t25\t0\t0\t0\n"
    assert dp.window_rows(got, A2I)[:2] == [("c1", 0, 7, 9, 7), ("c1", 7, 14, 10, 7)]
    assert dp.window_rows(got, A2I)[5] == ("c1", 196, 200, 5, 4)  # the last window ends at L
    wide = dp.depth(HAND, A2I, 0.5, window=1000)
    assert wide.windows == {"c1": [(0, 31, 25)], "c2": [(0, 30, 30)], "d1": [(0, 18, 18)]} and wide.per == got.per
    assert dp.window_rows(wide, A2I) == [("c1", 0, 200, 31, 25), ("c2", 0, 300, 30, 30), ("d1", 0, 500, 18, 18)]
    assert dp.depth(HAND, A2I, 0.5).windows == {}
    got0 = dp.depth(HAND, A2I, 0.0)  # the soft-clipped insertion counts and has no reference base: one more unplaced
    assert got0.unplaced == 6 and got0.per["c1"][0] == 6


def test_small_statistics_by_hand():
    assert dp.stats({3: 1}) == dp.Stats(1, Fraction(3), 3, Fraction(3), Fraction(0), 3, 1, 0, 0, 0)
    # L = 20: t = 1, ranks 1..18 of 0 x10, 5 x9, 40 x1 -> the single 40 and one 0 are trimmed; the median is rank 9, a 0
    s = dp.stats({0: 10, 5: 9, 40: 1})
    assert (s.median, s.trimmed, s.max, s.ge1, s.ge5, s.ge10, s.ge30) == (0, Fraction(45, 18), 40, 10, 10, 1, 1)
    assert dp.stats({0: 9, 5: 10, 40: 1}).median == 5  # rank 9 is the first 5
    assert dp.stats({0: 9, 7: 10}).trimmed == Fraction(70, 19)  # L = 19: t = 0
    assert dp.stats({}) == dp.Stats(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("seed", range(6))
def test_definition_against_a_per_base_array(seed):
    lengths, placed = dc.random_case(seed)
    assert set(dc.EDGE_LENGTHS) >= {1, 19, 20, 21, 39, 40, 41} and {n % 2 for n in lengths.values()} == {0, 1}
    for window in (0, 1, 7, 1000):
        per, unplaced, windows = dp.accumulate(placed, lengths, window)
        b_per, b_unplaced, b_windows, arrays = dc.brute(placed, lengths, window)
        assert (per, unplaced, windows) == (b_per, b_unplaced, b_windows)
    assert len(per["flat"][1]) == 1 and max(per["deep"][1]) == dp.CAP  # one bin; the clamp at work
    for acc, a in arrays.items():
        c = np.sort(np.minimum(a, dp.CAP))
        n = len(c)
        t = n * 5 // 100
        s = dp.stats(per[acc][1])
        assert s.length == n == sum(per[acc][1].values())
        # numpy's float64 sums of at most 5000 integers below 2^12 are exact; its variance rounds ~n times
        assert float(s.mean) == c.mean() and float(s.trimmed) == c[t:n - t].mean()
        assert float(s.variance) == pytest.approx(c.var(), rel=1e-11, abs=1e-11)
        assert s.median == c[(n - 1) // 2] and s.max == c[-1]
        assert [s.ge1, s.ge5, s.ge10, s.ge30] == [int((c >= k).sum()) for k in (1, 5, 10, 30)]


def test_clamp_histogram_clamped_windows_not():
    lengths = {"x": 300}
    per, unplaced, windows = dp.accumulate([("x", 100, 50)] * 5000, lengths, 20)
    assert per == {"x": [5000, {0: 250, dp.CAP: 50}]} and unplaced == 0
    s = dp.stats(per["x"][1])
    assert s.max == 4095 and s.mean == Fraction(4095 * 50, 300)  # the clamped mean
    assert windows == {"x": [(5, 5000 * 20, 20), (6, 5000 * 20, 20), (7, 5000 * 10, 10)]}  # the true sums


def test_invariants_with_coverage_on_the_same_lines():
    import coverage_cases as cc
    _, _, acc2info, taxid2info, _, lines = cc.case(300, 150)
    for pct in (0.0, 0.5, 0.95):
        cov, dep = cv.coverage(lines, acc2info, pct), dp.depth(lines, acc2info, pct, window=97)
        assert dep.unplaced == cov.unplaced and dep.lengths == cov.lengths and set(dep.per) == set(cov.per) and len(dep.per) > 3
        for acc, (aln, H) in dep.per.items():
            s = dp.stats(H)
            assert aln == cov.per[acc][0] and s.ge1 == cov.per[acc][2] and s.length == cov.lengths[acc]
            assert s.max < dp.CAP
            assert sum(c * n for c, n in H.items()) == cov.per[acc][1] == sum(w[1] for w in dep.windows[acc])
            assert sum(w[2] for w in dep.windows[acc]) == cov.per[acc][2]
        crow, drow = cv.rows(cov, acc2info, taxid2info), dp.rows(dep, acc2info, taxid2info)
        assert [r[:4] for r in crow] == [r[:4] for r in drow]  # the same rows in the same order
        for c, d in zip(crow, drow):
            assert sum(d[4].values()) == c[3] and dp.stats(d[4]).ge1 == c[6]


def test_lines_the_tokeniser_raises_on_still_raise():
    for line, exc in ((L("a", 0, "nope", 1, "4M"), KeyError), (L("a", 0, "c1", 1, "4="), ValueError),
                      ("a\t0\tc1\t1\t60\t4M\t*\t0\t0\tACGT\t*\n", IndexError), (L("a", 0, "c1", 1, "M"), ZeroDivisionError),
                      (L("a", "x", "c1", 1, "4M"), ValueError), (L("a", 0, "c1", 1, "4M", tag="NM:i:x"), ValueError)):
        with pytest.raises(exc):
            dp.depth([line], A2I, 0.5)


def test_exact_bytes_of_both_files_two_inputs(tmp_path):
    got = dp.depth(HEAD + [L("a", 0, "c1", 1, "10M"), L("b", 0, "c1", 6, "10M"), L("c", 0, "c1", 0, "1M")], A2I, 0.5, window=8)
    path, wpath = str(tmp_path / "depth.tsv"), str(tmp_path / "win.tsv")
    dp.write_depth(path)
    dp.write_depth(path, dp.rows(got, A2I, T2I), got.unplaced, source="one.sam", append=True)
    dp.write_depth(path, [], 0, source="two.bam", append=True)
    # c1: {0: 185, 1: 10, 2: 5}: mean 20 / 200, variance 30 / 200 - 0.01, t = 10 -> ranks 10..189: five 1s among 180
    want = ("#kind\tid\ttaxid\tlength\tmean_depth\tmedian_depth\ttrimmed_mean_depth\tdepth_variance\tmax_depth\tbases_ge_1\tbases_ge_5"
            "\tbases_ge_10\tbases_ge_30\n"
            "#file\tone.sam\n"
            "S\tc1\tg1.1\t200\t0.100000\t0\t0.027778\t0.140000\t2\t15\t0\t0\t0\n"
            "G\tg1.1\tg1.1\t1500\t0.013333\t0\t0.000000\t0.019822\t2\t15\t0\t0\t0\n"
            "#unplaced\t1\n"
            "#file\ttwo.bam\n"
            "#unplaced\t0\n")
    assert open(path).read() == want
    dp.write_windows(wpath)
    dp.write_windows(wpath, dp.window_rows(got, A2I), source="one.sam", append=True)
    dp.write_windows(wpath, [], source="two.bam", append=True)
    assert open(wpath).read() == ("#accession\tstart\tend\tmean_depth\tcovered_bases\n"
                                  "#file\tone.sam\n"
                                  "c1\t0\t8\t1.375000\t8\n"
                                  "c1\t8\t16\t1.125000\t7\n"
                                  "#file\ttwo.bam\n")
    dp.write_windows(wpath, dp.window_rows(got, A2I))  # one input file: no #file line
    assert open(wpath).read() == "#accession\tstart\tend\tmean_depth\tcovered_bases\nc1\t0\t8\t1.375000\t8\nc1\t8\t16\t1.125000\t7\n"
    assert dp.HEADER == want.split("\n")[0] + "\n"


def test_the_flags_exist_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        assert acts["depth"].default == "NONE" and acts["depth"].option_strings == ["--depth"]
        assert acts["depth_windows"].default == "NONE" and acts["depth_windows"].option_strings == ["--depth_windows"]
        assert acts["depth_window_size"].default == 1000 and acts["depth_window_size"].type is int
        args = cli.parser_for(tool).parse_args((["x.sam", "data"] if tool == "map_and_profile" else ["r.fq", "data"])
                                               + ["--depth_windows", "w.tsv", "--depth_window_size", "25"])
        assert (args.depth, args.depth_windows, args.depth_window_size) == ("NONE", "w.tsv", 25)


def test_map_main_refuses_two_processes_paf_and_a_window_below_one(monkeypatch, tmp_path):
    import stage_c_checks as sc
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    out, win = tmp_path / "depth.tsv", tmp_path / "win.tsv"

    def refused(infile, extra):
        args = sc.make_args(str(tmp_path / infile), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)
        with pytest.raises(SystemExit) as e:
            mp.map_main(args)
        assert "\n" not in str(e.value.code) and not out.exists() and not win.exists()
        return str(e.value.code)

    for extra in ({"depth": str(out)}, {"depth_windows": str(win)}):
        assert "PAF" in refused("x.paf", dict(extra, input_type="AUTO"))
    assert refused("x.sam", {"depth": str(out), "depth_window_size": 0}) == "Error: --depth_window_size must be at least 1."
    assert "at least 1" in refused("x.sam", {"depth_windows": str(win), "depth_window_size": -3})
    monkeypatch.setenv("WORLD_SIZE", "2")
    for extra in ({"depth": str(out)}, {"depth_windows": str(win)}):
        assert refused("x.sam", extra) == ("Error: --depth and --depth_windows run in one process on one GPU; start it without "
                                           "torch.distributed.run.")


# ---- mg_depth_core.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("depth") / "host_depth_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_depth_check.cpp")])
    return out


def _check(exe, tmp_path, lengths, placed, window):
    blob, accs = dc.case_blob(lengths, placed, window)
    p = tmp_path / "case.bin"
    p.write_bytes(blob)
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return dc.parse_check_output(out.stdout.decode(), accs)


@pytest.mark.parametrize("seed", range(3))
def test_core_header_serial_device_algorithm_equals_the_definition(exe, tmp_path, seed):
    lengths, placed = dc.random_case(seed)
    for window in (0, 1, 7, 1000):
        assert _check(exe, tmp_path, lengths, placed, window) == dp.accumulate(placed, lengths, window)


def test_core_header_accessions_of_length_0_and_1(exe, tmp_path):
    lengths = {"z0": 0, "one": 1, "z1": 0, "two": 2, "z2": 0}
    placed = [("one", 0, 1), ("one", 0, 9), ("one", 1, 1), ("z0", 0, 5), ("z1", 0, 1), ("two", 1, 1), ("two", 0, 0), ("z2", 3, 3)]
    got = _check(exe, tmp_path, lengths, placed, 1)
    assert got == dp.accumulate(placed, lengths, 1) == ({"one": [2, {2: 1}], "two": [1, {0: 1, 1: 1}]}, 5,
                                                        {"one": [(0, 2, 1)], "two": [(1, 1, 1)]})
    assert _check(exe, tmp_path, {}, [], 5) == ({}, 0, {})
