"""CPU: metalign_amd/variants.py (the definition of --variants / --variant_sites) against a hand table, and mg_variants_core.h —
the scalar walks of a SAM line and a BAM record and the site rule — on the host under the sanitizers."""
import os
import struct
import subprocess
from fractions import Fraction

import pytest

import variants_cases as vc
from metalign_amd import cli
from metalign_amd import coverage as cv
from metalign_amd import variants as var

HERE = os.path.dirname(os.path.abspath(__file__))
P = var.Params(5, 2, 50)


def test_hand_table_what_each_line_says_by_itself():
    assert var.MAX_PILE_SPAN == 2 ** 21 - 1 and (var.OTHER, var.GAP) == (4, 5)
    for ln, want in zip(vc.HAND, vc.HAND_WANT):
        f = cv.retained_fields(ln)
        assert (f is None) == (want is None), ln
        if f is not None:
            assert var.bases_of(f) == tuple(want), ln
    assert [var.code_of(b) for b in b"AaCcGgTtNRn*=."] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 4, 4]


def test_hand_table_counts_sums_and_sites():
    lengths = cv.lengths_of([], vc.A2I)
    piles = []
    for ln in vc.HAND:
        f = cv.retained_fields(ln)
        if f is not None and cv.counts(int(f[1]), *cv.matched_total(f), 0.5):
            piles.append((f[2],) + var.bases_of(f))
    n, aln, unpiled = var.accumulate(piles, lengths)
    assert n == vc.HAND_COUNTS and aln == vc.HAND_ALIGNMENTS and unpiled == vc.HAND_UNPILED
    got = var.variants(vc.HAND, vc.A2I, 0.5)
    assert got.per == vc.HAND_PER and got.sites == vc.HAND_SITES and got.unpiled == vc.HAND_UNPILED and got.lengths == lengths
    assert var.variants(vc.HAND, vc.A2I, 0.5, P) == got  # (the defaults)
    # D = 4 makes site 3 of c1 callable too: [0, 1, 1, 2], pairs 12, same 2 -> discordant 10; nobody but T has 2
    assert var.variants(vc.HAND, vc.A2I, 0.5, var.Params(4, 2, 50)).per["c1"] == [9, 5, 1, 134, 82]
    # C = 1: every second allele of the callable sites is a variant (1000 >= 50 d up to d = 20)
    assert var.variants(vc.HAND, vc.A2I, 0.5, var.Params(5, 1, 50)).per["c1"] == [9, 4, 4, 122, 72]
    # pct_id 0.4 lets r in (T on sites 0 and 1), 0 lets nothing more in
    assert var.variants(vc.HAND, vc.A2I, 0.4).per["c1"][0] == 10


def test_span_at_and_above_the_largest_pile():
    for line, piled in ((vc.SPAN_MAX, True), (vc.SPAN_OVER, False)):
        f = cv.retained_fields(line)
        pos0, span, codes = var.bases_of(f)
        assert (span == var.MAX_PILE_SPAN and codes[0] == 0 and set(codes[1:]) == {5}) if piled else (pos0, span, codes) == (0, 0, [])
        got = var.variants([line], vc.A2I, 0.0)
        assert (got.unpiled, got.per.get("c2", [0])[0]) == ((0, 1) if piled else (1, 0))
        assert var.variants([line], vc.A2I, 0.5).per == {} and var.variants([line], vc.A2I, 0.5).unpiled == 0  # (it does not count)


@pytest.mark.parametrize("n4, dcf, want", vc.SITE_CASES)
def test_the_site_rule_at_its_edges(n4, dcf, want):
    assert var.site_of(n4, var.Params(*dcf)) == want


def test_parameters_and_their_ranges():
    assert var.params() == (5, 2, 50) and var.params(2, 1, 0.5) == (2, 1, 500) and var.params(9, 9, 0.0) == (9, 9, 0)
    assert var.params(5, 2, 0.0125).permille == 12 and var.params(5, 2, 0.0135).permille == 14  # int(round(freq * 1000))
    for bad in ((1, 2, 0.05), (5, 0, 0.05), (5, 2, -0.001), (5, 2, 0.501)):
        with pytest.raises(ValueError):
            var.params(*bad)


def test_pack_and_unpack_and_the_side_array():
    assert var.pack([0, 1, 2]) == bytes([0x10, 0x02]) and var.pack([]) == b"" and var.pack([5, 4]) == bytes([0x45])
    assert var.unpack(var.pack([3, 5, 4, 0, 1]), 5) == [3, 5, 4, 0, 1]
    fields = [f for f in map(cv.retained_fields, vc.HAND) if f is not None]
    entries, pool = var.entries_and_pool(fields)
    assert entries[:3] == [(0, 0, 5), (3, 0, 3), (5, 1, 4)] and entries[7] == (0, 0, 0)  # (a: 3 bytes, b: 2; h is not piled)
    assert len(pool) == sum((s + 1) // 2 for _, _, s in entries)
    for (off, pos0, span), f in zip(entries, fields):
        assert (pos0, span, var.unpack(pool[off:off + (span + 1) // 2], span)) == var.bases_of(f)


def test_records_give_what_the_lines_give():
    from metalign_amd import _hip, map_and_profile as mp
    import numpy as np
    recs = mp.tokenise_sam(vc.HAND, vc.ACC_INDEX)
    entries, pool = var.entries_and_pool(f for f in map(cv.retained_fields, vc.HAND) if f is not None)
    names = ["Unmapped", "c1", "c2", "d1"]
    lengths = cv.lengths_of([], vc.A2I)
    got = var.variants_of_records(recs, np.array(entries, dtype=_hip.BASES_DTYPE), pool, names, lengths, 0.5)
    assert got == var.variants(vc.HAND, vc.A2I, 0.5)
    short = var.variants_of_records(recs, entries, pool, names[:2], lengths, 0.5)  # rows 2 and 3 are beyond the accessions
    assert short.unpiled == vc.HAND_UNPILED + 2 and set(short.per) == {"c1"}


def test_exact_bytes_of_both_files_one_and_two_inputs(tmp_path):
    got = var.variants(vc.HAND, vc.A2I, 0.5)
    rows = var.rows(got, vc.A2I, vc.T2I)
    path, sites = str(tmp_path / "v.tsv"), str(tmp_path / "s.tsv")
    var.write_variants(path, P)
    var.write_variants(path, P, rows, got.unpiled, append=True)
    var.write_sites(sites, P)
    var.write_sites(sites, P, got.sites, append=True)
    assert open(path).read() == vc.HAND_FILE and open(sites).read() == vc.HAND_SITES_FILE
    assert var.ratios(4, 1, 122, 72) == (Fraction(36, 61), Fraction(250)) and var.ratios(0, 0, 0, 0) == (0, 0)
    var.write_variants(path, P)
    var.write_sites(sites, P)
    for src in ("a.sam", "b.bam"):
        var.write_variants(path, P, rows, got.unpiled, source=src, append=True)
        var.write_sites(sites, P, got.sites, source=src, append=True)
    head, body = vc.HAND_FILE.split("\n", 2)[:2], vc.HAND_FILE.split("\n", 2)[2]
    assert open(path).read() == "\n".join(head) + "\n" + "#file\ta.sam\n" + body + "#file\tb.bam\n" + body
    shead, sbody = vc.HAND_SITES_FILE.split("\n", 2)[:2], vc.HAND_SITES_FILE.split("\n", 2)[2]
    assert open(sites).read() == "\n".join(shead) + "\n" + "#file\ta.sam\n" + sbody + "#file\tb.bam\n" + sbody


def test_lines_the_tokeniser_raises_on_still_raise():
    for line, exc in ((vc.L("a", 0, "nope", 1, "4M", "ACGT"), KeyError), (vc.L("a", 0, "c1", 1, "4=", "ACGT"), ValueError),
                      (vc.L("a", 0, "c1", 1, "4M", "ACGT", tags=()), IndexError), (vc.L("a", 0, "c1", 1, "M", "ACGT"), ZeroDivisionError),
                      (vc.L("a", "x", "c1", 1, "4M", "ACGT"), ValueError)):
        with pytest.raises(exc):
            var.variants([line], vc.A2I, 0.5)


def test_the_flags_exist_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        for flag in ("variants", "variant_sites"):
            assert acts[flag].default == "NONE" and acts[flag].option_strings == ["--" + flag]
        assert (acts["variant_min_depth"].default, acts["variant_min_count"].default, acts["variant_min_freq"].default) == (5, 2, 0.05)
        assert acts["variant_min_depth"].type is int and acts["variant_min_count"].type is int and acts["variant_min_freq"].type is float
        args = cli.parser_for(tool).parse_args((["x.sam", "data"] if tool == "map_and_profile" else ["r.fq", "data"])
                                               + ["--variant_sites", "s.tsv", "--variant_min_freq", "0.1"])
        assert (args.variants, args.variant_sites, args.variant_min_freq, args.identity) == ("NONE", "s.tsv", 0.1, "NONE")


def test_the_descriptor_is_the_last_family_and_reads_the_bases(tmp_path):
    import stage_c_checks as sc
    from metalign_amd import side_outputs as so
    assert so.FAMILIES[-1] is so.VARIANTS and so.VARIANTS.flags == ("variants", "variant_sites") and so.VARIANTS.side == "bases"
    args = sc.make_args("x.sam", "db_info.txt", "o.cami", {"variant_sites": str(tmp_path / "s.tsv")})
    sides = so.SideOutputs.of(args, "x.sam", header=lambda: ["@SQ\tSN:c1\tLN:7\n"])
    assert sides and sides.based and sides.sized and not sides.placed and not sides.edited and sides.header == ["@SQ\tSN:c1\tLN:7\n"]
    lengths = {"a": 1000, "b": 24}
    assert sides.need_bytes(lengths, 2, 10) == 16 * 1024 + 40 * 2 + 96 * 10
    assert not so.SideOutputs.of(sc.make_args("x.sam", "db_info.txt", "o.cami", {}), "x.sam").based
    so.write_headers(args)
    assert (tmp_path / "s.tsv").read_text() == "\n".join(vc.HAND_SITES_FILE.split("\n")[:2]) + "\n"
    args.side_reads = "unique"
    so.write_headers(args)
    assert (tmp_path / "s.tsv").read_text().endswith("#reads\tunique\n")


def test_map_main_refuses_two_processes_paf_and_parameters_out_of_range(monkeypatch, tmp_path):
    import stage_c_checks as sc
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    out = tmp_path / "variants.tsv"

    def refused(infile, extra):
        args = sc.make_args(str(tmp_path / infile), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)
        with pytest.raises(SystemExit) as e:
            mp.map_main(args)
        assert "\n" not in str(e.value.code) and not out.exists()
        return str(e.value.code)

    for flag in ("variants", "variant_sites"):
        assert refused("x.paf", {flag: str(out), "input_type": "AUTO"}) == (
            "Error: --variants and --variant_sites need SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.")
    assert "PAF" in refused("x.sam", {"variants": str(out), "paf_input": True})
    assert refused("x.sam", {"variants": str(out), "variant_min_depth": 1}) == "Error: --variant_min_depth must be at least 2."
    assert refused("x.sam", {"variants": str(out), "variant_min_count": 0}) == "Error: --variant_min_count must be at least 1."
    for freq in (-0.01, 0.51):
        assert refused("x.sam", {"variant_sites": str(out), "variant_min_freq": freq}) == "Error: --variant_min_freq must lie within 0 to 0.5."
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert refused("x.sam", {"variants": str(out)}) == ("Error: --variants and --variant_sites run in one process on one GPU; start it "
                                                        "without torch.distributed.run.")


# ---- mg_variants_core.h on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("variants") / "host_variants_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_variants_check.cpp")])
    return out


def _sam_case(line, want):
    """A line without its newline: the heap block ends exactly with the line."""
    raw = (line if isinstance(line, bytes) else line.encode()).rstrip(b"\n")
    f = raw.split(b"\t")
    cb = sum(len(x) + 1 for x in f[:5])
    sb = sum(len(x) + 1 for x in f[:9])
    pos0, span, codes = want
    return struct.pack("<7I", 0, len(raw), cb, cb + len(f[5]), sb, sb + len(f[9]), span) + bytes(codes) + raw


def _bam_case(rec, want):
    pos0, span, codes = want
    return struct.pack("<7I", 1, len(rec), 36, 0, 0, 0, span) + bytes(codes) + rec


def _site_case(n4, dcf, want):
    ok, major, var_alleles, pairs, disc = want
    return struct.pack("<10I2Q", *n4, *dcf, int(ok), major, sum(1 << a for a in var_alleles), pairs, disc)


def _run(exe, tmp_path, cases, sites=()):
    p = tmp_path / "cases.bin"
    p.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases) + struct.pack("<I", len(sites)) + b"".join(sites))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.decode().splitlines()[-1] == "%d cases, %d sites, 0 differ" % (len(cases), len(sites))


def test_core_header_sam_walk_on_the_hand_table(exe, tmp_path):
    # (a line without a place — k, l — never reaches the core's walk: the place is the tokeniser's, mg_coverage_core.h)
    cases = [_sam_case(ln, w) for ln, w in zip(vc.HAND, vc.HAND_WANT) if w is not None and cv.placement(cv.retained_fields(ln))[1]]
    # a SEQ that ends the line (no QUAL, no tags behind it): the last byte the walk may read is the line's last
    for cigar, seq, codes in (("5M", "ACGTA", [0, 1, 2, 3, 0]), ("1S3M1S", "ACGTA", [1, 2, 3]), ("5M", "ACGT", []), ("4M", "ACGTA", []),
                              ("2M2D1M", "ACG", [0, 1, 5, 5, 2]), ("1M2097150N", "A", None), ("1M2097151N", "A", [])):
        raw = ("q\t0\tc1\t1\t60\t%s\t*\t0\t0\t%s" % (cigar, seq)).encode()
        if codes is None:
            codes = [0] + [5] * (var.MAX_PILE_SPAN - 1)
        cases.append(_sam_case(raw, (0, len(codes), codes)))
    assert len(cases) > 20
    _run(exe, tmp_path, cases)


def test_core_header_bam_walk_on_the_hand_table(exe, tmp_path):
    cases = [_bam_case(rec, w) for rec, w, placed in vc.hand_bam_cases() if placed]
    assert len(cases) > 15 and any(w[1] % 2 for _, w, _ in vc.hand_bam_cases())
    # l_seq 0 is `*`; ops 5 (H), 6 (P) and 7 (=) give nothing; a record that ends with its SEQ (no QUAL: the fixed part lies about
    # nothing else) is walked to its last byte and no further
    cases.append(_bam_case(vc.bam_record("z", 0, 0, 0, "3M", "*"), vc.NOT_PILED))
    cases.append(_bam_case(vc.bam_record("z", 0, 0, 0, "1H2M1P1M1H", "ACG"), (0, 3, [0, 1, 2])))
    rec = vc.bam_record("z", 0, 0, 0, "3M", "TGA")
    rec = struct.pack("<I", len(rec) - 4 - 3) + rec[4:-3]  # without its three QUAL bytes
    cases.append(_bam_case(rec, (0, 3, [3, 2, 0])))
    rec = struct.pack("<I", len(rec) - 4 - 1) + rec[4:-1]  # ... and without the second SEQ byte: not piled, and not read
    cases.append(_bam_case(rec, vc.NOT_PILED))
    _run(exe, tmp_path, cases)


def test_core_header_site_rule(exe, tmp_path):
    sites = [_site_case(*c) for c in vc.SITE_CASES]
    sites.append(_site_case([2 ** 32 - 1, 2 ** 32 - 1, 0, 0], (5, 2, 50),
                            (True, 0, [1], (2 ** 33 - 2) * (2 ** 33 - 3) % 2 ** 64,
                             ((2 ** 33 - 2) * (2 ** 33 - 3) - 2 * (2 ** 32 - 1) * (2 ** 32 - 2)) % 2 ** 64)))  # (sums wrap in 64 bits)
    for n4 in vc.HAND_COUNTS["c1"].values():
        sites.append(_site_case(n4, tuple(P), var.site_of(n4, P)))
    _run(exe, tmp_path, [], sites)
