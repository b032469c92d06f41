"""CPU: metalign_amd/refdiff.py (the pileup against the reference: --ani, --vcf) against hand-worked sites, rows and files, mgvar::diff_of
on the host under the sanitizers, and the flags: parsed, wired into the VARIANTS family and refused as specified."""
import itertools
import struct
from fractions import Fraction

import pytest

import refdiff_cases as rc
import stage_c_checks as sc
import variants_cases as vc
from metalign_amd import cli
from metalign_amd import coverage as cv
from metalign_amd import refdiff as rd
from metalign_amd import refseq as rs
from metalign_amd import side_outputs as so
from metalign_amd import variants as var
from test_refseq_host import exe, run_check  # noqa: F401  (the fixture that compiles tests/host_refdiff_check.cpp)

P = rc.P

# The hand table of variants_cases over A2I (c1 20, c2 1000, d1 8).  c1's counts: 0 [5,0,0,1]  1 [1,5,0,1]  2 [0,2,3,1]  3 [0,1,1,2]
# 4 [1,1,1,2]  5 [0,0,1,1]; at (5, 2, 50) sites 0, 1, 2 and 4 are callable.  The reference: c1 = ACCNA + 15 A, c2 = 1000 A, d1 has none.
#   0 A = major A                          compared
#   1 C = major C                          compared
#   2 C: major G, C is a variant allele    compared, con_sub, emitted: ALT G, DP 6, AD 2,3, AF 0.5
#   3 N: depth 4                           not callable (at D = 4: ref_other)
#   4 A: major T, nothing else present     compared, con_sub, pop_sub, emitted: ALT T, DP 5, AD 1,2, AF 0.4
REF_FASTA = b">c1 the first\nACCNA\naaaaaaaaaaaaaaa\n>c2\n" + rc.wrap(b"A" * 1000, 60) + b">elsewhere\nACGT\n"
ANI_FILE = (rd.HEADER + "#min_depth\t5\tmin_count\t2\tmin_freq_permille\t50\n"
            "S\tc1\tg1.1\t20\t9\t4\t4\t2\t1\t0\t0.500000\t0.750000\n"
            "S\tc2\tg1.1\t1000\t1\t0\t0\t0\t0\t0\t0.000000\t0.000000\n"
            "G\tg1.1\tg1.1\t1020\t10\t4\t4\t2\t1\t0\t0.500000\t0.750000\n"
            "#unpiled\t%d\n#no_reference\t1\n" % vc.HAND_UNPILED)
VCF_FILE = ("##fileformat=VCFv4.2\n##source=metalign_amd\n##reference=ref.fa\n##contig=<ID=c1,length=20>\n##contig=<ID=c2,length=1000>\n"
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads with A, C, G or T at the site">\n'
            '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads per allele, the reference allele first">\n'
            '##INFO=<ID=AF,Number=A,Type=Float,Description="Share of DP per alternative allele">\n'
            "##metalign_variants=min_depth=5,min_count=2,min_freq_permille=50,reads=all\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "c1\t3\t.\tC\tG\t.\tPASS\tDP=6;AD=2,3;AF=0.500000\n"
            "c1\t5\t.\tA\tT\t.\tPASS\tDP=5;AD=1,2;AF=0.400000\n")


def _hand_ref():
    index = {a: i for i, a in enumerate(vc.A2I)}
    lengths = cv.lengths_of([], vc.A2I)
    parsed = rs.parse(REF_FASTA, index, [lengths[a] for a in vc.A2I])
    assert tuple(parsed.counters) == (3, 2, 1, 0, 0)
    return rd.ref_by_accession(parsed, index)


@pytest.mark.parametrize("case", rc.CLASSES)
def test_every_site_class(case):
    (n4, r), (compared, other, con, pop, emitted, alts) = case
    assert rd.diff_of(n4, r, P) == (bool(compared), bool(other), bool(con), bool(pop), bool(emitted), alts)


def test_emitted_is_a_con_sub_or_a_polymorphic_site():
    for n4 in itertools.product(range(0, 7, 2), repeat=4):
        for r in range(5):
            for p in (P, rc.LOW):
                d = rd.diff_of(list(n4), r, p)
                ok, major, alleles, _, _ = var.site_of(list(n4), p)
                assert d.emitted == (d.compared and (d.con_sub or bool(alleles))) and (not d.pop_sub or d.con_sub)
                assert d.compared + d.ref_other == int(ok) and set(d.alts) == ({major} | set(alleles)) - {r} if d.compared else not d.alts


def test_hand_table_figures_rows_and_both_files(tmp_path):
    ref = _hand_ref()
    assert set(ref) == {"c1", "c2"} and ref["c1"][:5] == bytes([0, 1, 1, 4, 0])
    got = rd.refdiff(vc.HAND, vc.A2I, 0.5, ref)
    assert got.per == {"c1": [9, 4, 4, 2, 1, 0, 2], "c2": [1, 0, 0, 0, 0, 0, 0]} and got.no_reference == 1
    assert got.sites == [("c1", 2, (0, 2, 3, 1), 1), ("c1", 4, (1, 1, 1, 2), 0)] and got.unpiled == vc.HAND_UNPILED
    rows = rd.rows(got, vc.A2I, vc.T2I)
    assert [r[:2] for r in rows] == [("S", "c1"), ("S", "c2"), ("G", "g1.1")] and rows[2][3:] == (1020, 10, 4, 4, 2, 1, 0)
    assert rd.ani(4, 2, 1) == (Fraction(1, 2), Fraction(3, 4)) and rd.ani(0, 0, 0) == (0, 0)
    path = str(tmp_path / "ani.tsv")
    rd.write_ani(path, P)
    rd.write_ani(path, P, rows, got.unpiled, got.no_reference, append=True)
    assert open(path).read() == ANI_FILE
    rd.write_ani(path, P, rows, got.unpiled, got.no_reference, source="b.bam", append=True)
    assert open(path).read() == ANI_FILE + "#file\tb.bam\n" + ANI_FILE.split("\n", 2)[2]
    assert rd.format_vcf(got, "ref.fa", vc.A2I, P) == VCF_FILE
    assert "reads=unique\n" in rd.format_vcf(got, "ref.fa", vc.A2I, P, unique=True)
    # D = 4: site 3 [0, 1, 1, 2] becomes callable, over a reference N
    assert rd.refdiff(vc.HAND, vc.A2I, 0.5, ref, var.Params(4, 2, 50)).per["c1"] == [9, 5, 4, 2, 1, 1, 2]


def test_alt_order_with_ties_and_af_formatting():
    p = rc.LOW
    line = rd.format_vcf_site(("x", 9, (3, 3, 3, 0), 3), p)
    assert line == "x\t10\t.\tT\tA,C,G\t.\tPASS\tDP=9;AD=0,3,3,3;AF=0.333333,0.333333,0.333333\n"
    assert rd.format_vcf_site(("x", 0, (0, 2, 3, 3), 0), p).split("\t")[4:] == ["G,T,C", ".", "PASS", "DP=8;AD=0,3,3,2;AF=0.375000,0.375000,0.250000\n"]
    assert rd.format_vcf_site(("x", 0, (1, 0, 2, 0), 0), p).endswith("\tA\tG\t.\tPASS\tDP=3;AD=1,2;AF=0.666667\n")
    assert rd.format_vcf_site(("x", 0, (0, 0, 0, 7), 1), p).endswith("\tC\tT\t.\tPASS\tDP=7;AD=0,7;AF=1.000000\n")


def test_a_genome_sums_its_accessions_and_skips_those_without_a_reference():
    a2i = {"a": [4, "t1", "", ""], "b": [4, "t1", "", ""], "c": [4, "t2", "", ""], "d": [4, "t1", "", ""]}
    t2i = {"t1": [12], "t2": [4]}
    n = {acc: {0: [0, 6, 0, 0], 1: [6, 0, 0, 0], 2: [2, 5, 0, 0]} for acc in a2i}
    aln = {"a": 3, "b": 2, "c": 1, "d": 5}
    lengths = {acc: 4 for acc in a2i}
    ref = {"a": bytes(4), "b": bytes([0, 0, 0, 4]), "c": bytes(4)}  # d has none
    got = rd.compare(n, aln, 7, lengths, list(a2i), ref, P)
    assert got.per["a"] == [3, 3, 3, 2, 1, 0, 2] and got.per["b"] == [2, 3, 3, 2, 1, 0, 2] and got.no_reference == 1 and "d" not in got.per
    rows = rd.rows(got, a2i, t2i)
    assert [r[1] for r in rows] == ["a", "b", "c", "t1", "t2"]
    assert rows[3] == ("G", "t1", "t1", 12, 5, 6, 6, 4, 2, 0) and rows[4] == ("G", "t2", "t2", 4, 1, 3, 3, 2, 1, 0)
    assert rd.format_row(rows[3]).endswith("\t0.333333\t0.666667\n")
    assert rd.format_vcf(got, "r.fa", a2i, P).count("##contig=") == 3 and "ID=d," not in rd.format_vcf(got, "r.fa", a2i, P)


def test_core_header_diff_rule(exe, tmp_path):  # noqa: F811
    sites = []
    for n4 in itertools.product((0, 1, 2, 3, 5, 9), repeat=4):
        for r in range(5):
            for p in (P, rc.LOW, var.Params(3, 1, 500)):
                d = rd.diff_of(list(n4), r, p)
                want = d.compared | d.ref_other << 1 | d.con_sub << 2 | d.pop_sub << 3 | d.emitted << 4
                sites.append(struct.pack("<9I", *n4, r, *p, want))
    for (n4, r), w in rc.CLASSES:
        sites.append(struct.pack("<9I", *n4, r, *P, w[0] | w[1] << 1 | w[2] << 2 | w[3] << 3 | w[4] << 4))
    sites.append(struct.pack("<9I", 2 ** 32 - 1, 2 ** 32 - 1, 0, 0, 1, *P, 1 | 4 | 16))  # (a tie at the top of the range: A is major, r = C a variant allele)
    sites.append(struct.pack("<9I", 9, 0, 0, 0, 255, *P, 2))  # (any code from 4 on is OTHER)
    run_check(exe, tmp_path, [], sites)


# ---- the flags ----------------------------------------------------------------------------------------------------------------
def test_the_flags_exist_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        assert (acts["ani"].default, acts["vcf"].default, acts["reference"].default) == ("NONE", "NONE", "AUTO")
        args = cli.parser_for(tool).parse_args((["x.sam", "data"] if tool == "map_and_profile" else ["r.fq", "data"])
                                               + ["--ani", "a.tsv", "--reference", "r.fa.gz"])
        assert (args.ani, args.vcf, args.reference, args.consensus) == ("a.tsv", "NONE", "r.fa.gz", "NONE")


def test_ani_and_vcf_open_the_variants_family_by_themselves(tmp_path):
    ref = tmp_path / "ref.fa"
    ref.write_bytes(REF_FASTA)
    for flag in ("ani", "vcf"):
        args = sc.make_args("x.sam", "db_info.txt", "o.cami", {flag: str(tmp_path / flag), "reference": str(ref)})
        assert so.VARIANTS.wanted(args) and so.VARIANTS.reference(args) == str(ref)
        sides = so.SideOutputs.of(args, "x.sam", header=lambda: ["@SQ\tSN:c1\tLN:7\n"])
        assert sides.families == (so.VARIANTS,) and sides.based and sides.sized
        lengths = {"a": 1000, "b": 24}
        text = len(REF_FASTA)
        assert sides.need_bytes(lengths, 2, 10) == 16 * 1024 + 40 * 2 + 96 * 10 + 1024 + 32 * 2 + text + 40 * (text // 60 + 1)
    args = sc.make_args("x.sam", "db_info.txt", "o.cami", {"ani": str(tmp_path / "a.tsv"), "vcf": str(tmp_path / "v.vcf"), "db": str(ref)})
    assert so.VARIANTS.reference(args) == str(ref)  # --reference AUTO: the database FASTA
    so.check_flags(args)
    so.write_headers(args)
    assert (tmp_path / "a.tsv").read_text() == "\n".join(ANI_FILE.split("\n")[:2]) + "\n" and (tmp_path / "v.vcf").read_text() == ""
    args.side_reads = "unique"
    so.write_headers(args)
    assert (tmp_path / "a.tsv").read_text().endswith("#reads\tunique\n") and (tmp_path / "v.vcf").read_text() == ""
    assert so.VARIANTS.reference(sc.make_args("x.sam", "d", "o", {"ani": "a"})) is None


def test_the_definition_writes_both_files_over_a_line_stream(tmp_path):
    ref = tmp_path / "ref.fa"
    ref.write_bytes(REF_FASTA)
    args = sc.make_args("x.sam", "db_info.txt", "o.cami", {"ani": str(tmp_path / "a.tsv"), "vcf": str(tmp_path / "v.vcf"),
                                                           "reference": str(ref)})
    so.write_headers(args)
    so.SideOutputs.of(args, "x.sam").append_from_definition("x.sam", lambda: iter(vc.HAND), vc.A2I, vc.T2I)
    assert (tmp_path / "a.tsv").read_text() == ANI_FILE
    assert (tmp_path / "v.vcf").read_text() == VCF_FILE.replace("##reference=ref.fa", "##reference=%s" % ref)


def test_map_main_refuses_before_a_gpu_is_touched(monkeypatch, tmp_path):
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    ref = tmp_path / "ref.fa"
    ref.write_bytes(REF_FASTA)
    out = tmp_path / "out.file"

    def refused(infile, extra, infiles=None):
        args = sc.make_args(str(tmp_path / infile), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)
        if infiles:
            args.infiles = [str(tmp_path / f) for f in infiles]
        with pytest.raises(SystemExit) as e:
            mp.map_main(args)
        assert "\n" not in str(e.value.code) and not out.exists()
        return str(e.value.code)

    for flag in ("ani", "vcf"):
        assert refused("x.sam", {flag: str(out)}) == so.VARIANTS.refuse_no_reference  # (SAM input: no --db either)
        missing = str(tmp_path / "nowhere.fa")
        assert refused("x.sam", {flag: str(out), "reference": missing}) == so.VARIANTS.refuse_reference_missing % missing
        assert refused("x.sam", {flag: str(out), "db": missing}) == so.VARIANTS.refuse_reference_missing % missing
        assert refused("x.paf", {flag: str(out), "reference": str(ref), "input_type": "AUTO"}) == (
            "Error: --%s needs SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns." % flag)
    assert "one by one" in refused("x.sam", {"vcf": str(out), "reference": str(ref)}, infiles=["x.sam", "y.sam"])
    assert "--variants and --variant_sites" in refused("x.paf", {"vcf": str(out), "variants": str(tmp_path / "t"), "reference": str(ref),
                                                                 "input_type": "AUTO"})
    monkeypatch.setenv("WORLD_SIZE", "2")
    for flag in ("ani", "vcf"):
        assert refused("x.sam", {flag: str(out), "reference": str(ref)}) == (
            "Error: --%s runs in one process on one GPU; start it without torch.distributed.run." % flag)


def test_metalign_resolves_the_reference_once_its_stages_have_written_the_database():
    args = cli.parser_for("metalign").parse_args(["r.fq", "data", "--ani", "a.tsv"])
    so.VARIANTS.check_reference(args)  # (no --db on this tool: wired to temp_dir/cmashed_db.fna behind the check)
    args.db = "tmp/cmashed_db.fna"
    assert so.VARIANTS.reference(args) == "tmp/cmashed_db.fna"
    args = cli.parser_for("metalign").parse_args(["r.fq", "data", "--vcf", "v.vcf", "--reference", "/nowhere/ref.fa"])
    with pytest.raises(SystemExit) as e:
        so.VARIANTS.check_reference(args)
    assert str(e.value.code) == so.VARIANTS.refuse_reference_missing % "/nowhere/ref.fa"
