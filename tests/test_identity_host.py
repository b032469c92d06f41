"""--identity on the host: the definition (metalign_amd/identity.py) against a hand table and an independent restatement, its
invariant with coverage.py, the exact bytes of the file, the SAM scanner and the BAM aux walk of mg_identity_core.h run under the
sanitizers, the flags and map_main's refusals."""
import os
import re
import struct
import subprocess
from fractions import Fraction

import pytest

import bamgen
import identity_cases as ic
from metalign_amd import bam, cli
from metalign_amd import coverage as cv
from metalign_amd import identity as idn

HERE = os.path.dirname(os.path.abspath(__file__))
A2I, T2I, L = ic.A2I, ic.T2I, ic.L
NONE = 2 ** 32 - 1


def test_hand_table_edits():
    """(nm, cols) of every retained line of the hand table, worked out by hand."""
    got = [idn.edit_of(f) for f in map(cv.retained_fields, ic.HAND) if f is not None]
    assert got == [(0, 10), (1, 10), (2, 10), (NONE, 10), (NONE, 10), (3, 10), (7, 100), (NONE, 10), (NONE, 10), (NONE, 10), (25, 10),
                   (0, 0), (9, 20), (0, 10), (0, 4), (1, 10), (2 ** 32 - 2, 10), (NONE, 10), (0, 10), (NONE, 10), (1, 10), (0, 8), (4, 10)]
    assert idn.NONE == NONE and idn.BINS == 1001


def test_hand_table_sums_histograms_and_statistics():
    got = idn.identity(ic.HAND, A2I, 0.5)
    # c1: a b c f g r v scored (bins 1000 900 800 700 930 0 900), d e h i j s u unscored; n and o do not count
    assert got.unscored == 7
    assert got.per == {"c1": [7, 160, 24, {1000: 1, 900: 2, 800: 1, 700: 1, 930: 1, 0: 1}],
                       "c2": [2, 30, 19, {0: 1, 550: 1}],                       # k: e = min(25, 10); m: (20 - 9) * 1000 // 20
                       "d1": [4, 38, 5, {900: 1, 1000: 2, 600: 1}]}             # p t w x
    rows = idn.rows(got, A2I, T2I)
    assert [r[:6] for r in rows] == [("S", "c1", "g1.1", 7, 160, 24), ("S", "c2", "g1.1", 2, 30, 19), ("S", "d1", "g2", 4, 38, 5),
                                     ("G", "g1.1", "g1.1", 9, 190, 43), ("G", "g2", "g2", 4, 38, 5)]
    assert rows[3][6] == {1000: 1, 900: 2, 800: 1, 700: 1, 930: 1, 0: 2, 550: 1}
    # c1 ascending: 0 700 800 900 900 930 1000 -> rank 3 is 900, rank 0 is 0
    assert idn.stats(*rows[0][4:]) == idn.Stats(1 - Fraction(24, 160), 900, 0, 4, 1, 1, 1)
    # g1.1 ascending: 0 0 550 700 800 900 900 930 1000 -> rank 4 is 800
    assert idn.stats(*rows[3][4:]) == idn.Stats(1 - Fraction(43, 190), 800, 0, 4, 1, 1, 1)
    # d1 ascending: 600 900 1000 1000 -> rank 1 is 900, rank 0 is 600
    assert idn.stats(*rows[2][4:]) == idn.Stats(1 - Fraction(5, 38), 900, 600, 3, 2, 2, 2)
    assert idn.format_row(rows[0]) == "S\tc1\tg1.1\t7\t160\t24\t0.850000\t0.900\t0.000\t4\t1\t1\t1\n"
    assert idn.format_row(rows[1]) == "S\tc2\tg1.1\t2\t30\t19\t0.366667\t0.000\t0.000\t0\t0\t0\t0\n"
    assert idn.format_row(rows[4]) == "G\tg2\tg2\t4\t38\t5\t0.868421\t0.900\t0.600\t3\t2\t2\t2\n"
    got0 = idn.identity(ic.HAND, A2I, 0.0)  # l counts and has no column: unscored; o counts: (0, 4), bin 1000
    assert got0.unscored == 8 and got0.per["c1"] == [8, 164, 24, {1000: 2, 900: 2, 800: 1, 700: 1, 930: 1, 0: 1}]
    assert got0.per["c2"] == got.per["c2"] and got0.per["d1"] == got.per["d1"]


def test_small_statistics_by_hand():
    assert idn.stats(0, 0, {}) == idn.Stats(0, 0, 0, 0, 0, 0, 0)
    assert idn.stats(10, 0, {1000: 1}) == idn.Stats(Fraction(1), 1000, 1000, 1, 1, 1, 1)
    # n = 20: the median is rank 9, p10 rank 2
    s = idn.stats(2000, 100, {500: 2, 900: 8, 950: 5, 970: 3, 990: 1, 1000: 1})
    assert s == idn.Stats(Fraction(19, 20), 900, 900, 18, 10, 5, 2)
    assert idn.stats(200, 0, {500: 3, 900: 7, 950: 10}).p10 == 500 and idn.stats(200, 0, {500: 2, 900: 8, 950: 11}).p10 == 900
    assert idn.stats(1, 0, {3: 10, 7: 10}).median == 3 and idn.stats(1, 0, {3: 10, 7: 11}).median == 7


# ---- an independent restatement: a regular expression over the raw line, a per-alignment list sorted for the ranks ---------------
_WS = " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"
_NM = re.compile(r"(?:^|(?<=[%s]))NM:i:([^%s]*)" % (_WS, _WS))
_VALUE = re.compile(r"[+-]?[0-9]+\Z")


def _restated(lines, acc2info, pct_id):
    """-> ({accession: [(cols, e)]}, unscored)"""
    per, unscored = {}, 0
    for line in lines:
        line = line.decode() if isinstance(line, bytes) else line
        if line.startswith("@"):
            continue
        parts = re.findall(r"[^%s]+" % _WS, line)
        if len(parts) < 6 or int(parts[1]) & 4 or parts[5] == "*":
            continue
        ops = re.findall(r"([0-9]*)([A-Za-z])", parts[5])
        matched = sum(int(n or 0) for n, op in ops if op == "M")
        total = sum(int(n or 0) for n, op in ops)
        if int(parts[1]) & 2048 or matched / total < pct_id:
            continue
        cols = sum(int(n or 0) for n, op in ops if op in "MIDX")
        # the text behind the eleventh field, scanned as one string
        m11 = re.match(r"[%s]*(?:[^%s]+[%s]+){11}" % (_WS, _WS, _WS), line)
        hit = _NM.search(line[m11.end():]) if m11 else None
        nm = None
        if hit and _VALUE.match(hit.group(1)) and 0 <= int(hit.group(1)) <= 2 ** 32 - 2:
            nm = int(hit.group(1))
        if nm is None or cols == 0:
            unscored += 1
            continue
        per.setdefault(parts[2], []).append((cols, min(nm, cols)))
    return per, unscored


@pytest.mark.parametrize("seed", range(5))
def test_definition_against_the_restatement(seed):
    _, accs, acc2info, taxid2info, _, lines = ic.case(250, 120, seed=seed, bam_safe=False)
    lines = lines + ic.HAND[2:]
    acc2info = dict(acc2info, **{a: A2I[a] for a in ("c1", "c2", "c3", "d1")})
    taxid2info = dict(taxid2info, **{"g1.1": [3000, "strain", "", ""], "g2": [500, "species", "", ""]})
    for pct in (0.0, 0.5, 0.95):
        got = idn.identity(lines, acc2info, pct)
        per, unscored = _restated(lines, acc2info, pct)
        assert got.unscored == unscored and set(got.per) == set(per) and (pct > 0.9 or len(per) > 6)
        for acc, alns in per.items():
            aln, columns, edits, H = got.per[acc]
            assert (aln, columns, edits) == (len(alns), sum(c for c, _ in alns), sum(e for _, e in alns))
            ids = sorted((c - e) * 1000 // c for c, e in alns)
            assert sorted(b for b, n in H.items() for _ in range(n)) == ids
            s = idn.stats(columns, edits, H)
            n = len(ids)
            assert (s.median, s.p10) == (ids[(n - 1) // 2], ids[n // 10])
            assert [s.ge900, s.ge950, s.ge970, s.ge990] == [sum(1 for b in ids if b >= k) for k in (900, 950, 970, 990)]
            assert s.identity == 1 - Fraction(edits, columns)
        if pct == 0.5:
            assert unscored > 30 and sum(len(a) for a in per.values()) > 300
            rows = idn.rows(got, acc2info, taxid2info)
            kinds = [r[0] for r in rows]
            assert kinds == sorted(kinds, reverse=True) and kinds.count("G") > 3  # the S rows, then the G rows
            for r in rows:
                if r[0] == "G":
                    mine = [x for x in rows if x[0] == "S" and x[2] == r[1]]
                    assert r[3:6] == tuple(sum(x[i] for x in mine) for i in (3, 4, 5)) and sum(r[6].values()) == r[3]


def test_scored_plus_unscored_are_the_lines_coverage_counts():
    _, _, acc2info, taxid2info, _, lines = ic.case(300, 150, bam_safe=False)
    for pct in (0.0, 0.5, 0.95):
        cov, got = cv.coverage(lines, acc2info, pct), idn.identity(lines, acc2info, pct)
        counted = sum(st[0] for st in cov.per.values()) + cov.unplaced
        assert sum(st[0] for st in got.per.values()) + got.unscored == counted > 100


def test_identity_of_records_equals_the_lines():
    from metalign_amd import map_and_profile as mp
    _, accs, acc2info, _, acc_index, lines = ic.case(200, 80)
    recs = mp.tokenise_sam(lines, acc_index)
    edits = [idn.edit_of(f) for f in map(cv.retained_fields, lines) if f is not None]
    names = [a for a, _ in sorted(acc_index.items(), key=lambda kv: kv[1])]
    assert len(recs) == len(edits)
    assert idn.identity_of_records(recs, edits, names, 0.5) == idn.identity(lines, acc2info, 0.5)
    short = idn.identity_of_records(recs, edits, names[:3], 0.5)  # rows beyond the accessions: unscored
    assert short.unscored > idn.identity(lines, acc2info, 0.5).unscored and set(short.per) <= set(names[:3])


def test_lines_the_tokeniser_raises_on_still_raise():
    for line, exc in ((L("a", 0, "nope", "4M", ["NM:i:0"]), KeyError), (L("a", 0, "c1", "4=", ["NM:i:0"]), ValueError),
                      (L("a", 0, "c1", "4M", []), IndexError), (L("a", 0, "c1", "M", ["NM:i:0"]), ZeroDivisionError),
                      (L("a", "x", "c1", "4M", ["NM:i:0"]), ValueError), (L("a", 0, "c1", "4M", ["NM:i:"]), ValueError)):
        with pytest.raises(exc):
            idn.identity([line], A2I, 0.5)


def test_exact_bytes_of_the_file_two_inputs(tmp_path):
    got = idn.identity(ic.HAND, A2I, 0.5)
    path = str(tmp_path / "identity.tsv")
    idn.write_identity(path)
    idn.write_identity(path, idn.rows(got, A2I, T2I), got.unscored, source="one.sam", append=True)
    idn.write_identity(path, [], 0, source="two.bam", append=True)
    want = ("#kind\tid\ttaxid\talignments\taligned_columns\tedit_distance\tidentity\tmedian_identity\tp10_identity\taln_ge_900\taln_ge_950"
            "\taln_ge_970\taln_ge_990\n"
            "#file\tone.sam\n"
            "S\tc1\tg1.1\t7\t160\t24\t0.850000\t0.900\t0.000\t4\t1\t1\t1\n"
            "S\tc2\tg1.1\t2\t30\t19\t0.366667\t0.000\t0.000\t0\t0\t0\t0\n"
            "S\td1\tg2\t4\t38\t5\t0.868421\t0.900\t0.600\t3\t2\t2\t2\n"
            "G\tg1.1\tg1.1\t9\t190\t43\t0.773684\t0.800\t0.000\t4\t1\t1\t1\n"
            "G\tg2\tg2\t4\t38\t5\t0.868421\t0.900\t0.600\t3\t2\t2\t2\n"
            "#unscored\t7\n"
            "#file\ttwo.bam\n"
            "#unscored\t0\n")
    assert open(path).read() == want
    idn.write_identity(path, idn.rows(got, A2I, T2I)[:1], 3)  # one input file: no #file line
    assert open(path).read() == want.split("\n")[0] + "\nS\tc1\tg1.1\t7\t160\t24\t0.850000\t0.900\t0.000\t4\t1\t1\t1\n#unscored\t3\n"
    assert idn.HEADER == want.split("\n")[0] + "\n"


def test_the_flag_exists_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        assert acts["identity"].default == "NONE" and acts["identity"].option_strings == ["--identity"]
        args = cli.parser_for(tool).parse_args((["x.sam", "data"] if tool == "map_and_profile" else ["r.fq", "data"])
                                               + ["--identity", "i.tsv"])
        assert args.identity == "i.tsv" and args.coverage == "NONE"


def test_map_main_refuses_two_processes_and_paf(monkeypatch, tmp_path):
    import stage_c_checks as sc
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    out = tmp_path / "identity.tsv"

    def refused(infile, extra):
        args = sc.make_args(str(tmp_path / infile), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)
        with pytest.raises(SystemExit) as e:
            mp.map_main(args)
        assert "\n" not in str(e.value.code) and not out.exists()
        return str(e.value.code)

    assert refused("x.paf", {"identity": str(out), "input_type": "AUTO"}).startswith("Error: --identity needs SAM or BAM alignments")
    assert "PAF" in refused("x.sam", {"identity": str(out), "paf_input": True})
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert refused("x.sam", {"identity": str(out)}) == ("Error: --identity runs in one process on one GPU; start it without "
                                                        "torch.distributed.run.")


# ---- mg_identity_core.h on the host -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("identity") / "host_identity_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_identity_check.cpp")])
    return out


def _sam_case(line):
    """A retained line -> its case: the offsets the parser leaves (the CIGAR field, the twelfth field) and the definition's edit."""
    raw = line if isinstance(line, bytes) else line.encode()
    raw = raw.rstrip(b"\n")
    spans = [m.span() for m in re.finditer(rb"[^ \t\n\r\x0b\x0c\x1c-\x1f]+", raw)]
    nm, cols = idn.edit_of(cv.retained_fields(line))
    return struct.pack("<6I", 0, len(raw), spans[5][0], spans[11][0] if len(spans) > 11 else len(raw), nm, cols) + raw


def _bam_case(record, want=None, names=(b"c1", b"c2", b"d1")):
    """A BAM record (block_size first) -> its case; want: (nm, cols), by default the definition over the record's SAM rendering."""
    if want is None:
        want = idn.edit_of(cv.retained_fields(bam.render(record[4:], list(names))))
    return struct.pack("<6I", 1, len(record), 36, 0, want[0], want[1]) + record


def _run(exe, tmp_path, cases):
    p = tmp_path / "cases.bin"
    p.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.decode().splitlines()[-1] == "%d cases, 0 differ" % len(cases)


def test_core_header_sam_scanner(exe, tmp_path):
    lines = [ln for ln in ic.HAND if cv.retained_fields(ln) is not None]
    for seed in (1, 2):
        lines += [ln for ln in ic.case(120, 60, seed=seed, bam_safe=False)[5] if cv.retained_fields(ln) is not None]
    lines += [L("z", 0, "c1", "4294967295M7I", ["NM:i:4294967294"]), L("z", 0, "c1", "99999999999999M", ["NM:i:1"]),
              L("z", 0, "c1", "3M", ["NM:i:5"]).rstrip("\n") + " ", L("z", 0, "c1", "3M", ["AS:i:1", "NM:i:"]),
              L("z", 0, "c1", "3M", ["AS:i:1", "NM:i"]), L("z", 0, "c1", "3M", ["AS:i:1", "N"]), L("z", 0, "c1", "3M", ["AS:i:1", "NM:i:+"]),
              L("z", 0, "c1", "3M", ["AS:i:1", "NM:i:4294967294"]), L("z", 0, "c1", "3M", ["AS:i:1", "NM:i:00000000000000000004294967294"])]
    cases = [_sam_case(ln) for ln in lines]
    edits = [struct.unpack_from("<2I", c, 16) for c in cases]
    assert len({e for e in edits}) > 40 and sum(1 for nm, _ in edits if nm == NONE) > 40 and (NONE, NONE) not in edits
    assert (2 ** 32 - 2, NONE) in edits and (1, NONE) in edits  # the sums saturate
    _run(exe, tmp_path, cases)


def _record(tags, cigar="10M", flag=0):
    return bamgen.record(L("r", flag, "c1", cigar, tags).rstrip("\n").split("\t"), 0, -1)


def _with_aux(raw_aux, cigar="10M"):
    """A record whose aux bytes are given as they are, its block_size covering them."""
    rec = _record([], cigar)
    body = rec[4:] + raw_aux
    return struct.pack("<I", len(body)) + body


def test_core_header_bam_aux_walk_every_type_in_front_of_nm(exe, tmp_path):
    front = ["XA:A:x", "Xc:i:-5", "XC:i:200", "Xs:i:-300", "XS:i:40000", "Xi:i:-70000", "XI:i:3000000000", "XF:f:1.5", "XZ:Z:hello",
             "XH:H:1AE3", "XB:B:c,1,-2", "XB:B:C,200,3", "XB:B:s,-300", "XB:B:S,1,2,3", "XB:B:i,-70000,1", "XB:B:I,5", "XB:B:f,1.5,2.5",
             "XB:B:C", "XZ:Z:"]
    cases = []
    for t in front:
        for nm in ("NM:i:3", "NM:i:300", "NM:i:70000", "NM:i:-1", "NM:i:-300", "NM:i:4294967294", "NM:i:4294967295", "NM:i:0"):
            cases.append(_bam_case(_record(["AS:i:1", t, nm, "ms:i:9"])))
    cases.append(_bam_case(_record(["AS:i:1"] + front + ["NM:i:2"])))
    cases.append(_bam_case(_record(["AS:i:1"] + front)))                      # none
    cases.append(_bam_case(_record(["NM:i:4"] + front)))                      # the first tag
    cases.append(_bam_case(_record(["NM:i:4", "NM:i:5"])))                    # the first wins
    for other in ("NM:Z:3", "NM:A:3", "NM:f:3", "NM:H:1A", "NM:B:c,3", "nm:i:3", "Nm:i:3", "NN:i:3", "MN:i:3"):
        cases.append(_bam_case(_record(["AS:i:1", other])))
        cases.append(_bam_case(_record(["AS:i:1", other, "NM:i:6"])))
    for cigar in ("5M2I3D4X6M", "10S5N", "3S4M2H", "7M1P7M", "268435455M268435455I268435455D"):
        cases.append(_bam_case(_record(["NM:i:1"], cigar)))
    wants = [struct.unpack_from("<2I", c, 16) for c in cases]
    assert (3, 10) in wants and (NONE, 10) in wants and (2 ** 32 - 2, 10) in wants and (1, 20) in wants and (1, 0) in wants
    assert (1, 3 * 268435455) in wants and (6, 10) in wants
    _run(exe, tmp_path, cases)


def test_core_header_bam_white_space_in_a_value_cuts_its_field(exe, tmp_path):
    cases = [
        _bam_case(_record(["AS:i:1", "XZ:Z:a b NM:i:77 c", "NM:i:2"])),       # a piece that starts with NM:i: comes first
        _bam_case(_record(["AS:i:1", "XZ:Z:a bNM:i:77 c", "NM:i:2"])),        # not at a piece's start
        _bam_case(_record(["AS:i:1", "XZ:Z:a NM:i:7x", "NM:i:2"])),           # malformed, and the search stops there
        _bam_case(_record(["AS:i:1", "XZ:Z:a NM:i:", "NM:i:2"])),             # empty: the value ends with the field
        _bam_case(_record(["AS:i:1", "XZ:Z:a NM:i:8", "NM:i:2"])),            # the value ends where the Z value ends
        _bam_case(_record(["AS:i:1", "XH:H:1A\x1fNM:i:9\x0b", "NM:i:2"])),
        _bam_case(_record(["AS:i:1", "XZ:Z:NM:i:5", "NM:i:2"])),              # XZ:Z:NM:i:5 is one field
        _bam_case(_record(["XZ:Z:12 NM:i:6", "NM:i:2"])),                     # in the first tag
        _bam_case(_with_aux(b"ASC\x01" + b"XAA " + b"NMC\x03"), (3, 10)),     # an A byte that is white space changes nothing here
        _bam_case(_with_aux(b"ASC\x01" + b" NC\x03"), (NONE, 10)),            # ' N:i:3': N:i:3 is a field, not NM:i:
        _bam_case(_with_aux(b"ASC\x01" + b"X\tZNM:i:4\0" + b"NMC\x03"), (3, 10)),  # tag 'X\t': the field ':Z:NM:i:4'
        _bam_case(_with_aux(b"ASC\x01" + b"XAAN" + b"M:C\x03"), (NONE, 10)),  # fields XA:A:N and M::i:3
    ]
    wants = [struct.unpack_from("<2I", c, 16)[0] for c in cases]
    assert wants == [77, 2, NONE, NONE, 8, 9, 2, 6, 3, NONE, 3, NONE]
    # (the rendering of the records bamgen can write agrees with the values written here)
    for tags, nm in ((["AS:i:1", "XZ:Z:a b NM:i:77 c", "NM:i:2"], 77), (["AS:i:1", "XZ:Z:a NM:i:7x", "NM:i:2"], NONE)):
        assert idn.edit_of(cv.retained_fields(bam.render(_record(tags)[4:], [b"c1"])))[0] == nm
    _run(exe, tmp_path, cases)


def test_core_header_bam_truncated_and_garbage_aux_at_the_records_end(exe, tmp_path):
    """The host renderer raises on these; the device walk ends with NONE — unless NM came first — and reads no byte at or behind
    the record's end (the case's heap block ends there: the sanitizer would report it)."""
    ok = b"ASC\x01"
    cases = [
        _bam_case(_with_aux(ok + b"NMi\x03\x00"), (NONE, 10)),                         # an int cut short
        _bam_case(_with_aux(ok + b"NM"), (NONE, 10)),                                  # two bytes
        _bam_case(_with_aux(ok + b"N"), (NONE, 10)),
        _bam_case(_with_aux(ok + b"NMC"), (NONE, 10)),                                 # the type and no value
        _bam_case(_with_aux(ok + b"XZZabc"), (NONE, 10)),                              # a Z value without its NUL
        _bam_case(_with_aux(ok + b"XZZab NM:i:5"), (NONE, 10)),                        # ... with a piece that looks like one
        _bam_case(_with_aux(ok + b"XBBc\xff\xff\xff\x7f\x01"), (NONE, 10)),            # a B array that claims 2^31 elements
        _bam_case(_with_aux(ok + b"XBBc\x02\x00"), (NONE, 10)),                        # a B header cut short
        _bam_case(_with_aux(ok + b"XBBq\x00\x00\x00\x00"), (NONE, 10)),                # a B subtype that does not exist
        _bam_case(_with_aux(ok + b"XQq\x00\x00\x00\x00" + b"NMC\x03"), (NONE, 10)),    # a type that does not exist
        _bam_case(_with_aux(ok + b"NMC\x03" + b"XZZabc"), (3, 10)),                    # NM first: the search was over
        _bam_case(_with_aux(ok + b"NMC\x03" + b"\xff"), (3, 10)),
        _bam_case(_with_aux(ok + b"XSs\x01"), (NONE, 10)),
        _bam_case(_with_aux(ok + b"XFf\x00\x00\x80"), (NONE, 10)),
        _bam_case(_with_aux(b""), (NONE, 10)),                                         # no aux field at all
        _bam_case(_with_aux(ok + b"\xff\xfe\xfd\xfc\xfb"), (NONE, 10)),
    ]
    _run(exe, tmp_path, cases)
