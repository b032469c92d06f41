"""CPU: the aligner's gapped extension (--align_band; metalign_amd/align.py: extend_gapped) against hand-worked tables, its records
against what stage C's definitions read back from its SAM text, band 0 against the ungapped aligner, the three flags,
mg_align_gap_core.h — the per-cell rules the kernel shares — on the host under the sanitizers, cell for cell and column for column,
and the planted-indel property on the definition alone."""
import os
import re
import struct
import subprocess

import pytest

import align_cases as ac
import align_gap_cases as gc
from metalign_amd import align, coverage, identity, map_and_profile, metalign, refseq, variants
from metalign_amd.side_outputs import align_gap_params, check_flags

HERE = os.path.dirname(os.path.abspath(__file__))

#      0         1         2         3         4         5
#      0123456789012345678901234567890123456789012345678901234
REF = b"ACGTTGCATGCCATGGTACCTTAGGACTGACTTACGGATCCATTGACCGTAAGCT"


def cigar_of(ops):
    return "".join("%d%s" % (len(m.group(0)), m.group(0)[0]) for m in re.finditer("M+|I+|D+", ops))


def run(read, ref, d, band, P=4, O=6, E=1):
    """-> (score, b, e, nm, pos0, span, CIGAR without clips)."""
    r = align.extend_gapped(refseq.codes_of(read), refseq.codes_of(ref), d, P, align.gap_params(band, O, E))
    return r[:6] + (cigar_of(r[6]),)


def test_hand_a_deletion_of_three_bases():
    """The read is REF without its bases 25 .. 27 (ACT): 52 bases.  On the diagonal d = 0 read base i meets reference base i, which
    matches for i < 25: H(24, 24) = 25.  Read bases 25 .. 51 are REF[28 ..]: they match on the diagonal j - i = 3, three offsets
    right of the band's centre, inside a band of 4.  Leaving (24, 24) along j costs O + 3 E = 9: D(24, 27) = 25 - 9 = 16, and the
    27 matches behind it give H(51, 54) = 16 + 27 = 43.  Staying on d = 0 instead meets GAC against ACT ...: no path without the gap
    reaches 43 (the scan's best is the 25 of the front).  No other three bases can be left out: REF[23:32] is GGACTGACT, and leaving
    out GAC (24 .. 26) or CTG (26 .. 28) leaves GTGA or GGAA where the read has GGGA.  The walk back takes 27 diagonals, the
    deletion (opened at (24, 25): D == H(24, 24) - 7), then 25 diagonals down to (0, 0), whose predecessor does not exist."""
    read = REF[:25] + REF[28:]
    assert len(REF) == 55 and REF[25:28] == b"ACT"
    assert run(read, REF, 0, 4) == (43, 0, 52, 3, 0, 55, "25M3D27M")
    # the candidate right of the gap (d = 3) finds the same alignment: what makes the two halves collapse in the selection
    assert run(read, REF, 3, 4) == (43, 0, 52, 3, 0, 55, "25M3D27M")
    # the ungapped scan on either diagonal: 25 and 27
    assert align.extend(refseq.codes_of(read), refseq.codes_of(REF), 0, 4)[:3] == (25, 0, 25)
    assert align.extend(refseq.codes_of(read), refseq.codes_of(REF), 3, 4)[:3] == (27, 25, 52)


def test_hand_the_mirror_insertion():
    """REF as the read, REF without ACT as the reference: the three bases are inserted.  I(27, 24) = H(24, 24) - 9 = 16 (opened at
    (25, 24), extended twice), then 27 matches on j - i = -3: 43 again; the read span is 55, the reference span 52."""
    assert run(REF, REF[:25] + REF[28:], 0, 4) == (43, 0, 55, 3, 0, 52, "25M3I27M")


def test_hand_a_gap_inside_a_homopolymer_goes_left():
    """Reference ... TACC AAAA GGAC ..., the read with AAA: any of the four A can be the one left out, every placement scores
    48 - 7 = 41.  The walk back prefers the diagonal wherever H == X, so it stays on the right-hand diagonal as long as that
    explains H, which is down to the FIRST A of the run: the deletion falls on reference base 20, the leftmost placement.  The
    mirror case inserts the read's first A of the run."""
    ref = b"ACGTTGCATGCCATGGTACCAAAAGGACTGACTTACGGATCCATTGACC"
    read = ref[:20] + b"AAA" + ref[24:]
    assert ref[20:24] == b"AAAA" and ref[19:20] != b"A" and ref[24:25] != b"A"
    assert run(read, ref, 0, 4) == (41, 0, 48, 1, 0, 49, "20M1D28M")
    assert run(ref, read, 0, 4) == (41, 0, 49, 1, 0, 48, "20M1I28M")


def test_hand_a_gap_as_long_as_the_band_is_found_and_one_longer_is_not():
    """Band 3.  Three bases left out: as at band 4.  Four left out (25 .. 28): the read goes on with REF[29:] = ACTTACGG ..., whose
    diagonal j - i = 4 is no cell of the band.  By chance its first three bases ACT equal REF[25:28], so the diagonal itself gives
    28 matches and then G against T: (28, 0, 28), ungapped.  The insertions mirror it."""
    three, four = REF[:25] + REF[28:], REF[:25] + REF[29:]
    assert four[25:29] == b"ACTT" and REF[25:29] == b"ACTG"
    assert run(three, REF, 0, 3) == (43, 0, 52, 3, 0, 55, "25M3D27M")
    assert run(four, REF, 0, 3) == (28, 0, 28, 0, 0, 28, "28M")
    assert run(REF, three, 0, 3) == (43, 0, 55, 3, 0, 52, "25M3I27M")
    assert run(REF, four, 0, 3) == (28, 0, 28, 0, 0, 28, "28M")
    # at band 4 it is found; REF[24:29] is GACTG, so leaving out GACT or ACTG gives the same read, and the walk goes left
    assert run(four, REF, 0, 4) == (41, 0, 51, 4, 0, 55, "24M4D27M")


def test_hand_gap_open_zero():
    """O = 0: the three-base deletion costs 3, 52 - 3 = 49.  And a mismatch (P = 4) is dearer than a deletion and an insertion of
    one base (1 + 1): read = 30 bases of REF with base 10 substituted scores 29 - 2 = 27 with both gaps, not 29 - 4 = 25.  Walking
    back from (11, 11) the diagonal does not explain H, the insertion (tried before the deletion) does: I, then D — forwards the
    deletion stands before the insertion."""
    assert run(REF[:25] + REF[28:], REF, 0, 4, O=0) == (49, 0, 52, 3, 0, 55, "25M3D27M")
    assert REF[10:11] != b"T"
    assert run(REF[:10] + b"T" + REF[11:30], REF[:30], 0, 2, O=0) == (27, 0, 30, 2, 0, 30, "10M1D1I19M")
    assert run(REF[:10] + b"T" + REF[11:30], REF[:30], 0, 2, O=6) == (25, 0, 30, 1, 0, 30, "30M")


def test_hand_two_gaps_in_one_read():
    """REF without bases 15, 16 and with a G in front of base 35: 15 + 18 + 20 = 53 matches, less (6 + 2) and (6 + 1): 38.  The path
    moves two offsets right of the centre and one back."""
    read = REF[:15] + REF[17:35] + b"G" + REF[35:]
    assert len(read) == 54
    assert run(read, REF, 0, 4) == (38, 0, 54, 3, 0, 55, "15M2D18M1I20M")


def test_hand_a_read_hanging_over_the_accessions_start():
    """d = -2: the read's first two bases have no cell at all (j < 0).  20 + 18 matches less 6 + 2: 30; b = 2, pos0 = 0."""
    assert run(b"GG" + REF[:20] + REF[22:40], REF, -2, 4) == (30, 2, 40, 2, 0, 40, "20M2D18M")
    # nothing aligns: score 0, no alignment
    assert run(b"AAAA", b"CCCC", 0, 2) == (0, 0, 0, 0, 0, 0, "")


def test_gap_parameter_ranges():
    assert align.gap_params() == (0, 6, 1) and align.gap_params(8) == (8, 6, 1) and align.gap_params(31, 0, 64) == (31, 0, 64)
    for bad, named in ((dict(band=-1), "--align_band"), (dict(band=32), "--align_band"), (dict(band=8, gap_open=-1), "--align_gap_open"),
                       (dict(band=8, gap_open=65), "--align_gap_open"), (dict(band=8, gap_extend=0), "--align_gap_extend"),
                       (dict(band=8, gap_extend=65), "--align_gap_extend")):
        with pytest.raises(ValueError) as e:
            align.gap_params(**bad)
        assert named in str(e.value)


# ---- the records and the SAM text -----------------------------------------------------------------------------------------------
def test_hand_records_and_sam_line_of_a_gapped_alignment():
    read = b"tt" + REF[:15] + REF[17:35] + b"G" + REF[35:50] + b"ccc"  # 2S 15M 2D 18M 1I 15M 3S, on strand 0 at pos0 = 100
    al = align.GapAln(0, 0, 98, 33, 2, 51, 3, 100, 50, "M" * 15 + "DD" + "M" * 18 + "I" + "M" * 15)
    recs, places, edits, entries, pool = align.records([read], [[al]])
    assert len(read) == 54 and recs.tolist() == [(0x80000000, 48, 54 + 2, 54 << 12)] and places.tolist() == [(100, 50)] and edits.tolist() == [(3, 51)]
    assert entries.tolist() == [(0, 100, 50)] and len(pool) == 25
    codes = [b & 15 if j % 2 == 0 else b >> 4 for j in range(50) for b in [pool[j // 2]]]
    assert codes == list(refseq.codes_of(REF[:15])) + [5, 5] + list(refseq.codes_of(REF[17:50]))
    line = align.sam_lines([b"r"], [read], None, ["acc"], [1000], [[al]])[-1]
    assert line == b"r\t0\tacc\t101\t255\t2S15M2D18M1I15M3S\t*\t0\t0\t" + read.translate(align._LETTER) + b"\t*\tNM:i:3\n"


def round_trip(seqs, alns, names, lengths):
    """records() against what stage C's definitions read from sam_lines()' text."""
    recs, places, edits, entries, pool = align.records(seqs, alns)
    lines = [ln for ln in align.sam_lines([b"q%d" % i for i in range(len(seqs))], seqs, None, names, lengths, alns) if not ln.startswith(b"@")]
    assert len(lines) == len(recs)
    seqs_of = [seq for seq, kept in zip(seqs, alns) for _ in kept]
    tk = map_and_profile._Tokeniser({n: i for i, n in enumerate(names)})  # the records themselves: what stage C reads from the text
    for ln in lines:
        tk.feed(ln.decode())
    assert tk.records().tolist() == recs.tolist()
    for r, ln in enumerate(lines):
        f = coverage.retained_fields(ln)
        assert coverage.placement(f) == tuple(places[r].tolist())
        assert identity.edit_of(f) == tuple(edits[r].tolist())
        cig = re.findall(r"(\d+)([MIDS])", f[5])
        assert sum(int(n) for n, op in cig if op == "M") == recs[r]["matched"]
        assert sum(int(n) for n, op in cig) == recs[r]["total"]  # (every operation, as map_and_profile's tokeniser counts a line)
        assert sum(int(n) for n, op in cig if op in "MIS") == len(seqs_of[r])
        pos0, span, codes = variants.bases_of(f)
        off, p0, sp = entries[r].tolist()
        if f[9] == "*":
            assert (span, sp) == (0, 0)
            continue
        assert (pos0, span) == (p0, sp)
        assert codes == [pool[off + j // 2] >> 4 if j % 2 else pool[off + j // 2] & 15 for j in range(sp)]
    return len(lines)


@pytest.mark.parametrize("band", gc.BANDS)
def test_records_round_trip_through_the_sam_text(band):
    gt = gc.table(band)
    names, seqs, alns, stats, refined = gc.batch_of(gt, len(gt.reads))
    assert variants.GAP == align.GAP_CODE
    assert round_trip(seqs, alns, gt.t.names, gt.t.lengths) > 150
    gapped = [al for kept in alns for al in kept if isinstance(al, align.GapAln)]
    assert sum("I" in al.ops for al in gapped) > 10 and sum("D" in al.ops for al in gapped) > 10


# ---- what exists stays ------------------------------------------------------------------------------------------------------------
def test_band_zero_is_the_ungapped_aligner():
    for k, w in ac.PARAMS:
        t = ac.table(k, w)
        for name, seq in t.reads:
            assert align.align_read_gapped(seq, t.index, t.ref, t.p, align.gap_params(0)) == (t.alns[name],) + t.stats_of[name] + (0,)


@pytest.mark.parametrize("band", gc.BANDS)
def test_a_refined_score_is_never_below_the_ungapped_one(band):
    """Every candidate of every case, accepted or not."""
    gt = gc.table(band)
    t, n = gt.t, 0
    for _, seq in gt.reads:
        codes = refseq.codes_of(seq)
        rc = align.revcomp_codes(codes)
        for a, strand, d in align.candidates(codes, t.index, t.p):
            o = rc if strand else codes
            score, b, e, nm = align.extend(o, t.ref.codes[a], d, t.p.mismatch)
            g = align.extend_gapped(o, t.ref.codes[a], d, t.p.mismatch, gt.gp)
            assert g[0] >= score
            if e - b == len(o) and score > 0:  # a full-length segment is the band's best too: nothing to refine
                assert g[:4] == (score, b, e, nm) and g[6] == "M" * len(o)
            n += 1
    assert n > 300


def test_the_case_table_holds_what_it_promises():
    gt8, gt1 = gc.table(8), gc.table(1)
    big = gt8.t.names.index("len70001")
    for kind in ("del", "ins"):
        found, missed = gt8.alns["%s_L150_g8_at75" % kind], gt8.alns["%s_L150_g9_at75" % kind]
        assert len(found) == 1 and (found[0].b, found[0].e) == (0, 150) and (kind[0].upper() * 8) in found[0].ops
        assert missed and all(x.e - x.b < 100 and "I" not in align.ops_of(x) and "D" not in align.ops_of(x) for x in missed)
    # the two halves of a read collapse to one alignment: two refined candidates, one record
    assert gt8.stats_of["del_L150_g8_at75"][2] == 2 and gt1.stats_of["del_L150_g1_at75"][2] == 2
    assert gt8.alns["two_gaps"][0].ops.count("D") == 3 and gt8.alns["two_gaps"][0].ops.count("I") == 2
    for name in ("across_gaps", "across_gaps2", "across_ins"):  # never across the boundary of two accessions
        assert {x.a for x in gt8.alns[name]} >= ({big} if name == "across_gaps2" else {gt8.t.names.index("len5000"), big})
        for x in gt8.alns[name]:
            assert 0 <= align.pos0_of(x) and align.pos0_of(x) + align.span_of(x) <= gt8.t.lengths[x.a]
    assert gt8.alns["gap_left1"][0].b == 1 and align.pos0_of(gt8.alns["gap_left1"][0]) == 0 and "D" in gt8.alns["gap_left1"][0].ops
    assert align.span_of(gt8.alns["longer_len64"][0]) == 64 and "D" in gt8.alns["longer_len64"][0].ops
    assert len(gt8.alns["tandem_del"]) < len(gt1.alns["tandem_del"])  # the band of 8 holds the 3-base gap, the band of 1 does not
    full = gt8.alns["del_L1024_g8_at512"][0]
    assert (full.b, full.e, full.span) == (0, 1024, 1032)
    for b in gc.BANDS:
        assert sum(v[2] for v in gc.table(b).stats_of.values()) > 200


# ---- the flags --------------------------------------------------------------------------------------------------------------------
PARSERS = [("map_and_profile", map_and_profile.profile_parseargs), ("metalign", metalign.metalign_parseargs)]


@pytest.mark.parametrize("tool,parse", PARSERS)
def test_the_flags_parse_with_their_defaults(tool, parse):
    a = parse(["reads.fq", "data"])
    assert (a.align_band, a.align_gap_open, a.align_gap_extend) == (0, 6, 1) and align_gap_params(a) == (0, 6, 1)
    a = parse(["reads.fq", "data", "--aligner", "device", "--align_band", "8", "--align_gap_open", "4", "--align_gap_extend", "2"])
    assert align_gap_params(a) == align.GapParams(8, 4, 2)
    check_flags(a)


@pytest.mark.parametrize("extra,named", [(["--align_band", "-1"], "--align_band"), (["--align_band", "32"], "--align_band"),
                                         (["--align_gap_open", "-1"], "--align_gap_open"), (["--align_gap_open", "65"], "--align_gap_open"),
                                         (["--align_gap_extend", "0"], "--align_gap_extend"), (["--align_gap_extend", "65"], "--align_gap_extend")])
@pytest.mark.parametrize("tool,parse", PARSERS)
def test_check_flags_refuses_values_out_of_range(tool, parse, extra, named):
    argv = ["reads.fq", "data", "--aligner", "device"] + (["--db", "db.fna"] if tool == "map_and_profile" else []) + extra
    with pytest.raises(SystemExit) as e:
        check_flags(parse(argv))
    assert str(e.value).startswith("Error: ") and named in str(e.value)
    check_flags(parse([x for x in argv if x not in ("--aligner", "device")]))  # only under --aligner device
    if tool == "map_and_profile":  # ... and only on reads
        check_flags(parse(["x.sam"] + argv[1:]))


# ---- mg_align_gap_core.h on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("align_gap") / "host_align_gap_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_align_gap_check.cpp")])
    return out


def run_check(exe, tmp_path, cases):
    """cases: (P, gp, d, read codes, reference codes) -> the program's [(result as extend_gapped gives it, rows as gap_cells)]."""
    blob = [struct.pack("<I", len(cases))]
    for P, gp, d, o, g in cases:
        blob.append(struct.pack("<IIIIiII", P, gp.band, gp.gap_open, gp.gap_extend, d, len(o), len(g)) + bytes(o) + bytes(g))
    p = tmp_path / "cases.bin"
    p.write_bytes(b"".join(blob))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d cases" % len(cases)
    got, rows = [], []
    for ln in lines[:-1]:
        f = ln.split()
        if f[0] == "r":
            rows.append([None if c == "-" else tuple(None if x == "n" else int(x) for x in c.split(",")) for c in f[2:]])
        else:
            got.append((tuple(int(x) for x in f[2:8]) + ("" if f[8] == "*" else f[8],), rows))
            rows = []
    return got


def check_against_the_definition(exe, tmp_path, cases):
    got = run_check(exe, tmp_path, cases)
    assert len(got) == len(cases)
    for (P, gp, d, o, g), (result, rows) in zip(cases, got):
        assert rows == align.gap_cells(o, g, d, P, gp)
        assert result == align.extend_gapped(o, g, d, P, gp)


def test_core_header_on_the_hand_cases(exe, tmp_path):
    c = refseq.codes_of
    three, two = REF[:25] + REF[28:], REF[:15] + REF[17:35] + b"G" + REF[35:]
    cases = [(4, align.gap_params(B, O, 1), d, c(read), c(ref))
             for B in (1, 3, 4, 31) for O in (0, 6) for d, read, ref in ((0, three, REF), (3, three, REF), (0, REF, three), (0, two, REF),
                                                                          (-2, b"GG" + REF[:20] + REF[22:40], REF), (40, REF, REF),
                                                                          (-54, REF, REF), (-60, REF, REF), (0, b"AAAA", b"CCCC"),
                                                                          (0, b"NNNN", b"NNNN"), (0, REF, b""))]
    check_against_the_definition(exe, tmp_path, cases)
    got = run_check(exe, tmp_path, cases[55:56])  # (band 4, O 6, the deletion on d = 0)
    assert got[0][0] == (43, 0, 52, 3, 0, 55, "M" * 25 + "DDD" + "M" * 27)


@pytest.mark.parametrize("band", gc.BANDS)
def test_core_header_against_the_definition_over_the_generators(exe, tmp_path, band):
    """Every accepted candidate of every case of the table, refined or not, and the other gap costs on every fifth."""
    gt = gc.table(band)
    t, cases = gt.t, []
    for _, seq in gt.reads:
        if len(seq) > 300 and band == 31:
            continue  # (the 1024-base rows at the widest band: 130 000 cells of text each; bands 1 and 8 carry that length)
        codes = refseq.codes_of(seq)
        rc = align.revcomp_codes(codes)
        for a, strand, d in sorted(align.candidates(codes, t.index, t.p)):
            o = rc if strand else codes
            if align.extend(o, t.ref.codes[a], d, t.p.mismatch)[0] < t.p.min_score:
                continue
            cases.append((t.p.mismatch, gt.gp, d, o, t.ref.codes[a]))
            if len(cases) % 5 == 0:
                cases.append((1, align.gap_params(band, 0, 2), d, o, t.ref.codes[a]))
                cases.append((64, align.gap_params(band, 64, 64), d, o, t.ref.codes[a]))
    assert len(cases) > 300
    check_against_the_definition(exe, tmp_path, cases)


# ---- the planted-indel property -------------------------------------------------------------------------------------------------
def test_planted_indels_are_found_with_the_band_and_not_without():
    """The generator of align_gap_cases.property_inputs: 300 reads of 150 bases with one indel of 1 .. 8 bases each and 2 %
    substitutions, every parameter at its default, band 8.  A read is found when its primary lies on its accession and covers at
    least 140 read bases: at least 285 of 300 with the band, at most 30 of 300 without.  Measured: 299 and 0."""
    names, lengths, fasta, ref, reads, truth = gc.property_inputs()
    assert len(reads) == 300 and all(len(s) == 150 for _, s in reads)
    seqs, p = [s for _, s in reads], align.params()
    index = align.build_index(ref, p.k, p.w)
    gapped, stats, refined = align.align_reads_gapped(seqs, ref, p, gc.gap_params_of(gc.PROPERTY_BAND), index=index)
    ungapped, stats0 = align.align_reads(seqs, ref, p, index=index)
    with_band = sum(gc.found(kept, a) for kept, a in zip(gapped, truth))
    without = sum(gc.found(kept, a) for kept, a in zip(ungapped, truth))
    print("found with band %d: %d of 300 (%d refined, %s); without: %d of 300 (%s)" % (gc.PROPERTY_BAND, with_band, refined, stats, without, stats0))
    assert with_band >= 285
    assert without <= 30
