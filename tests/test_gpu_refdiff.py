"""-m gpu: the reference FASTA parsed by record on the device (mg_refseq.hip) against metalign_amd/refseq.py, the pileup compared with
it (mg_variants_diff, mg_variants_fetch_diffs) against metalign_amd/refdiff.py, and --ani / --vcf through map_main.  Every
comparison is exact: integers and bytes."""
import gzip

import numpy as np
import pytest

import bamgen
import collate_cases
import consensus_cases as cc
import identity_cases as ic
import refdiff_cases as rc
import stage_c_checks as sc
import variants_cases as vc
from metalign_amd import _hip
from metalign_amd import collate
from metalign_amd import map_and_profile as mp
from metalign_amd import refdiff as rd
from metalign_amd import refseq as rs
from metalign_amd import side_outputs as so
from metalign_amd import side_reads as sr
from metalign_amd import variants as var

pytestmark = pytest.mark.gpu

PCT = 0.5
P, LOW = rc.P, rc.LOW
AROUND = b">\n>A\n"  # what lies around the text in memory: bytes that would open records if they were read


# ---- the parse ------------------------------------------------------------------------------------------------------------------
def _parse(hip, text, names, lengths, offset=0):
    """The text at `offset` bytes behind a 16-byte boundary, between bytes that are no part of it -> a RefSeq (the caller frees it)."""
    buf = np.frombuffer((AROUND * ((len(text) + 64) // len(AROUND) + 1))[:len(text) + 64], dtype=np.uint8).copy()
    buf[offset:offset + len(text)] = np.frombuffer(text, dtype=np.uint8)
    dev, index = hip.array(buf), hip.acc_index(names)
    try:
        assert dev.ptr % 16 == 0
        return hip.refseq_parse(dev.ptr + offset, len(text), index, lengths)
    finally:
        dev.free()
        index.free()


def _check(hip, text, names, lengths, offset=0):
    want = rs.parse(text, {a: i for i, a in enumerate(names)}, lengths)
    ref = _parse(hip, text, names, lengths, offset)
    try:
        assert ref.stats() == want.counters, (offset, ref.stats(), want.counters)
        assert ref.loaded().tolist() == want.loaded, offset
        got, flat = ref.download(), rs.flat(want, lengths)
        assert got == flat, (offset, next(i for i in range(len(flat)) if got[i] != flat[i]))
    finally:
        ref.free()
    return want


@pytest.mark.parametrize("width", rc.LINE_WIDTHS)
def test_line_widths_record_lengths_reversed_order_and_every_kind_in_between(hip, width):
    text, names, lengths = rc.geometry(width)
    assert lengths[:10] == [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 70001]
    want = _check(hip, text, names, lengths)
    assert tuple(want.counters) == (14, 10, 1, 1, 2) and want.loaded == [1] * 10 + [0]


@pytest.mark.parametrize("width", [16, 17])
def test_the_text_at_every_offset_from_a_16_byte_boundary(hip, width):
    """... with lines of 16 and 17 bases: the newlines fall in every byte of a window at every offset."""
    text, names, lengths = rc.geometry(width, lengths=[0, 1, 63, 64, 65, 1023, 1025])
    assert {i % 16 for i, b in enumerate(text) if b == 10} == set(range(16)) or width != 16
    for offset in range(16):
        _check(hip, text, names, lengths, offset)


def test_the_hand_table_and_every_prefix_of_it(hip):
    names = sorted(rc.HAND_INDEX, key=rc.HAND_INDEX.get)
    want = _check(hip, rc.HAND_TEXT, names, rc.HAND_LENGTHS)
    assert tuple(want.counters) == rc.HAND_COUNTERS and want.codes == rc.HAND_CODES
    for n in range(0, len(rc.HAND_TEXT), 3):  # a text that ends inside a header, a name, a line, behind a \r
        _check(hip, rc.HAND_TEXT[:n], names, rc.HAND_LENGTHS, offset=n % 16)


@pytest.mark.parametrize("name", sorted(rc.EDGE_TEXTS))
def test_a_header_last_headers_only_no_header_and_an_empty_file(hip, name):
    want = _check(hip, rc.EDGE_TEXTS[name], rc.EDGE_NAMES, rc.EDGE_LENGTHS, offset=5)
    assert name != "headers_only" or tuple(want.counters) == (4, 1, 1, 2, 0)
    assert name not in ("empty", "no_header") or tuple(want.counters) == (0, 0, 0, 0, 0)


def test_the_first_record_of_a_row_wins_whatever_the_grid(hip):
    """Five thousand records of one row, only the first of the right length: with any other winner the row is mismatched."""
    text = b">r\nACGT\n" + b"".join(b">r\nAC%s\n" % (b"G" * (i % 7)) for i in range(5000)) + b">s\nAC\n>s\nTT\n"
    want = _check(hip, text, ["r", "s"], [4, 2])
    assert tuple(want.counters) == (5003, 2, 0, 0, 5001) and want.codes == {0: bytes([0, 1, 2, 3]), 1: bytes([0, 1])}
    want = _check(hip, text[8:], ["r", "s"], [4, 2])  # without that first record: the first is `AC`, a mismatch
    assert tuple(want.counters) == (5002, 1, 0, 1, 5000)


def test_a_gz_reference_gives_the_codes_of_the_plain_file(hip, tmp_path):
    text, names, lengths = rc.geometry(60)
    (tmp_path / "r.fa").write_bytes(text)
    (tmp_path / "r.fa.gz").write_bytes(gzip.compress(text))
    (tmp_path / "empty.fa").write_bytes(b"")
    want = rs.parse(text, {a: i for i, a in enumerate(names)}, lengths)
    index = hip.acc_index(names)
    try:
        got = []
        for name in ("r.fa", "r.fa.gz"):
            ref = hip.refseq_from_file(str(tmp_path / name), index, lengths)
            got.append((ref.download(), ref.loaded().tolist(), ref.stats()))
            ref.free()
        assert got[0] == got[1] == (rs.flat(want, lengths), want.loaded, want.counters)
        ref = hip.refseq_from_file(str(tmp_path / "empty.fa"), index, lengths)
        assert ref.stats() == (0, 0, 0, 0, 0) and not ref.loaded().any() and set(ref.download()) == {255}
        ref.free()
        with pytest.raises(_hip.HipError) as e:  # lengths for another number of rows than the index has
            hip.refseq_parse(0, 0, index, lengths[:-1])
        assert e.value.code == _hip.ERR_ARG
    finally:
        index.free()


# ---- the comparison -------------------------------------------------------------------------------------------------------------
# nine rows of 1030 sites — a block of 1024 sites ends inside every one of them — whose shifts put every class at every position, and
# in between a row of length 0, one nobody hits, one without a reference and two short ones that share a block with their neighbours
LENGTHS = [1030, 1030, 0, 1030, 70, 1030, 1030, 66, 1030, 1030, 3, 1030, 1030, 5]
SHIFTS = [0, 1, 0, 2, 0, 3, 4, 0, 5, 6, 1, 7, 8, 2]
QUIET, NO_REF = 4, 7


class _Case:
    def __init__(self, hip):
        self.names = ["a%d" % i for i in range(len(LENGTHS))]
        self.len_of = dict(zip(self.names, LENGTHS))
        counts, self.codes = rc.class_counts(LENGTHS, SHIFTS, quiet=(QUIET,))
        self.recs, self.ent, self.pool = cc.records_of_counts(counts)
        self.n, self.aln, self.unpiled = var.counts_of_records(self.recs, self.ent, self.pool, self.names, self.len_of, PCT)
        self.fasta = rc.fasta_of(self.names, self.codes, skip=(NO_REF,))
        self.ref = _parse(hip, self.fasta, self.names, LENGTHS)
        self.dev = hip.variants(LENGTHS)
        try:
            self.dev.add(self.recs, self.ent, self.pool, PCT)
        except BaseException:
            self.free()
            raise

    def want(self, p):
        ref = {self.names[r]: c for r, c in self.codes.items() if r != NO_REF}
        return rd.compare(self.n, self.aln, self.unpiled, self.len_of, self.names, ref, p)

    def check(self, p):
        want = self.want(p)
        comp, con, pop, other, sites = self.dev.diff(self.ref, *p)
        for r, a in enumerate(self.names):
            st = want.per.get(a, [0] * 7)
            assert (int(comp[r]), int(con[r]), int(pop[r]), int(other[r])) == tuple(st[2:6]), (a, p)
        got = [(self.names[int(s["acc"])], int(s["pos0"]), tuple(int(x) for x in s["n"]), int(s["ref"])) for s in sites]
        assert got == want.sites, p
        return want

    def free(self):
        self.ref.free()
        self.dev.free()


@pytest.fixture(scope="module")
def case(hip):
    c = _Case(hip)
    yield c
    c.free()


@pytest.mark.parametrize("p", [P, LOW])
def test_every_site_class_at_the_edges_of_a_ballot_a_block_and_an_accession(case, p):
    assert case.ref.loaded().tolist() == [int(r != NO_REF) for r in range(len(LENGTHS))]  # (the quiet row and the empty one are loaded)
    want = case.check(p)
    assert want.no_reference == 1 and set(want.per) == {a for r, a in enumerate(case.names) if r not in (QUIET, NO_REF, 2)}
    if p == P:  # the table's own expectations: every class at every edge position, over the nine long rows
        full = [r for r, L in enumerate(LENGTHS) if L == 1030]
        emitted = {(s[0], s[1]) for s in want.sites}
        for pos in rc.EDGE_POSITIONS + [0, 1029]:
            classes = {(pos + SHIFTS[r]) % len(rc.CLASSES) for r in full}
            assert classes == set(range(len(rc.CLASSES)))
            for r in full:
                flags = rc.CLASSES[(pos + SHIFTS[r]) % len(rc.CLASSES)][1]
                assert ((case.names[r], pos) in emitted) == bool(flags[4])
        per_class = [sum(1 for pos in range(1030) if (pos + 0) % 9 == k) for k in range(9)]
        assert want.per["a0"][2:6] == [sum(per_class[k] * rc.CLASSES[k][1][f] for k in range(9)) for f in (0, 2, 3, 1)]


def test_finish_and_consensus_before_and_after_a_diff_give_what_they_gave(case):
    dev, rows = case.dev, list(range(len(LENGTHS)))
    before = dev.finish(*P)
    sites = dev.fetch_sites()
    text = dev.consensus(rows, *P, True)
    assert before[6] == len(sites) > 500
    case.check(LOW)
    assert np.array_equal(dev.fetch_sites(), sites)  # (the sites of the last finish, not the diff's)
    case.check(P)
    after = dev.finish(*P)
    assert all(np.array_equal(x, y) for x, y in zip(before[:5], after[:5])) and before[5:] == after[5:]
    assert np.array_equal(dev.fetch_sites(), sites) and dev.consensus(rows, *P, True) == text
    case.check(P)  # (and a diff after a finish)


def test_the_grid_cut_to_a_few_workgroups(case):
    full = case.dev.diff(case.ref, *P)
    for grid in (1, 2):
        _hip.debug_set("var_grid", grid)
        try:
            cut = case.dev.diff(case.ref, *P)
        finally:
            _hip.debug_set("var_grid", 0)
        assert all(np.array_equal(x, y) for x, y in zip(full, cut))
    assert len(full[4]) > 1000


def test_a_reference_for_other_rows_or_lengths_and_thresholds_out_of_range_are_refused(hip, case):
    def refused(ref, p):
        with pytest.raises(_hip.HipError) as e:
            case.dev.diff(ref, *p)
        assert e.value.code == _hip.ERR_ARG
        return str(e.value)

    fewer = _parse(hip, case.fasta, case.names[:-1], LENGTHS[:-1])
    other = _parse(hip, case.fasta, case.names, LENGTHS[:5] + [1031] + LENGTHS[6:])
    try:
        assert "13" in refused(fewer, P) and "1031" in refused(other, P)
        for bad in ((1, 2, 50), (5, 0, 50), (5, 2, 501)):
            refused(case.ref, var.Params(*bad))
    finally:
        fewer.free()
        other.free()
    fresh = hip.variants(LENGTHS)
    try:
        with pytest.raises(_hip.HipError) as e:  # no diff yet
            hip._chk(hip.lib.mg_variants_fetch_diffs(fresh.handle, None))
        assert e.value.code == _hip.ERR_STATE
        comp, con, pop, other_, sites = fresh.diff(case.ref, *P)  # no alignment anywhere: nothing compared
        assert not comp.any() and not other_.any() and len(sites) == 0
    finally:
        fresh.free()
    case.check(P)  # (the refusals left the accumulator as it was)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _reference_for(lines, dbinfo):
    """A FASTA for the bulk lines: per accession the sample's major allele, another base at every seventh site with a count, an N
    at every eleventh; lower case here and there; the third accession with a piled alignment left out, the fifth a base short."""
    args = sc.make_args("x.sam", dbinfo, "-", {})
    acc2info, _ = mp.get_acc2info(args)
    n, aln, _, lengths = var.counts_of_lines(lines, acc2info, PCT)
    out, hit = [], 0
    for acc in reversed(list(acc2info)):  # (not db_info's order)
        L = lengths[acc]
        if acc == "Unmapped":
            continue
        seq = bytearray(b"ACGT"[len(out) % 4:len(out) % 4 + 1] * L)
        for k, (pos, n4) in enumerate(sorted(n.get(acc, {}).items())):
            major = var.site_of(n4, LOW)[1]
            seq[pos] = ord("N") if k % 11 == 10 else b"ACGT"[(major + (k % 7 == 6)) % 4]
        if aln.get(acc):
            hit += 1
            if hit == 3:
                continue
            if hit == 5:
                seq = seq[:-1]
        body = rc.wrap(bytes(seq), 60)
        out.append(b">" + acc.encode() + b" from the sample\n" + (body.lower() if len(out) % 3 == 1 else body))
    assert hit > 10
    return b"".join(out)


def _definition(lines, dbinfo, ref_path, p=P, unique=False):
    args = sc.make_args("x.sam", dbinfo, "-", {})
    acc2info, taxid2info = mp.get_acc2info(args)
    if unique:
        lines = sr.unique_lines(lines, acc2info, PCT)
    n, aln, unpiled, lengths = var.counts_of_lines(lines, acc2info, PCT)
    order = list(acc2info)
    index = {a: i for i, a in enumerate(order)}
    parsed = rs.parse(rs.read_bytes(str(ref_path)), index, [lengths[a] for a in order])
    diff = rd.compare(n, aln, unpiled, lengths, order, rd.ref_by_accession(parsed, index), p)
    ani = (rd.HEADER + var.params_line(p) + (sr.HEADER_LINE if unique else "")
           + rd.format_block(rd.rows(diff, acc2info, taxid2info), diff.unpiled, diff.no_reference))
    return ani, rd.format_vcf(diff, str(ref_path), acc2info, p, unique), diff


def _run(path, dbinfo, tmp_path, tag, ref, flags=("ani", "vcf"), **extra):
    (tmp_path / tag).mkdir()
    outs = {f: tmp_path / tag / ("out." + f) for f in flags}
    mp.map_main(sc.make_args(str(path), dbinfo, str(tmp_path / tag / "out.cami"),
                             dict({"input_type": "sam", "db": "unused.fna", "sampleID": "s", "reference": str(ref)},
                                  **{f: str(o) for f, o in outs.items()}, **extra)))
    return tuple(outs[f].read_text() for f in flags)


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("refdiff_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = vc.dress(ic.dress(open(sam).read(), 52), 53)
    text = "".join(lines)
    (d / "b.sam").write_text(text)
    (d / "b.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "b.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    fasta = _reference_for(lines, dbinfo)
    (d / "ref.fa").write_bytes(fasta)
    (d / "ref.fa.gz").write_bytes(gzip.compress(fasta))
    return d, dbinfo, lines


@pytest.mark.parametrize("form", ["b.sam", "b.sam.gz", "b.bam"])
@pytest.mark.parametrize("ref", ["ref.fa", "ref.fa.gz"])
def test_map_main_gives_the_definitions_bytes(hip, bulk, tmp_path, form, ref):
    d, dbinfo, lines = bulk
    ani, vcf, diff = _definition(lines, dbinfo, d / ref)
    assert diff.no_reference == 2 and len(diff.per) > 8 and len(diff.sites) > 50  # (one left out, one a base short)
    assert sum(st[3] for st in diff.per.values()) > 10 and sum(st[5] for st in diff.per.values()) > 3
    assert _run(d / form, dbinfo, tmp_path, "both", d / ref) == (ani, vcf)


def test_map_main_each_flag_alone_and_beside_variants_and_consensus(hip, bulk, tmp_path):
    d, dbinfo, lines = bulk
    ani, vcf, _ = _definition(lines, dbinfo, d / "ref.fa")
    assert _run(d / "b.sam", dbinfo, tmp_path, "ani", d / "ref.fa", flags=("ani",)) == (ani,)
    assert _run(d / "b.bam", dbinfo, tmp_path, "vcf", d / "ref.fa", flags=("vcf",)) == (vcf,)
    alone = {}
    for f in ("variants", "consensus"):
        (tmp_path / f).mkdir()
        alone[f] = tmp_path / f / "out"
        mp.map_main(sc.make_args(str(d / "b.sam"), dbinfo, str(tmp_path / f / "o.cami"),
                                 {"input_type": "sam", "db": "unused.fna", "sampleID": "s", f: str(alone[f])}))
    v, c = tmp_path / "v.tsv", tmp_path / "c.fa"
    assert _run(d / "b.sam", dbinfo, tmp_path, "all", d / "ref.fa", variants=str(v), consensus=str(c)) == (ani, vcf)
    assert v.read_bytes() == alone["variants"].read_bytes() and c.read_bytes() == alone["consensus"].read_bytes()
    other = dict(variant_min_depth=3, variant_min_count=1, variant_min_freq=0.2)
    ani_o, vcf_o, _ = _definition(lines, dbinfo, d / "ref.fa", p=var.params(3, 1, 0.2))
    assert ani_o != ani and _run(d / "b.sam.gz", dbinfo, tmp_path, "other", d / "ref.fa", **other) == (ani_o, vcf_o)


def test_map_main_unique_reads_and_a_coordinate_sorted_copy(hip, bulk, tmp_path):
    d, dbinfo, lines = bulk
    ani, vcf, _ = _definition(lines, dbinfo, d / "ref.fa")
    ani_u, vcf_u, _ = _definition(lines, dbinfo, d / "ref.fa", unique=True)
    assert ani_u != ani and "#reads\tunique\n" in ani_u and ",reads=unique\n" in vcf_u
    assert _run(d / "b.sam", dbinfo, tmp_path, "unique", d / "ref.fa", side_reads="unique") == (ani_u, vcf_u)
    shuffled = collate_cases.coordinate_shuffle("".join(lines))
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam("".join(shuffled), block=20000))
    ani_s, vcf_s, _ = _definition(shuffled, dbinfo, d / "ref.fa.gz")  # (the definition over the lines the file holds)
    assert _run(tmp_path / "s.bam", dbinfo, tmp_path, "sorted", d / "ref.fa.gz", collate="always") == (ani_s, vcf_s)
    ani_su, vcf_su, _ = _definition(list(collate.collated_lines(shuffled)), dbinfo, d / "ref.fa.gz", unique=True)
    assert _run(tmp_path / "s.bam", dbinfo, tmp_path, "sorted_unique", d / "ref.fa.gz", collate="always",
                side_reads="unique") == (ani_su, vcf_su)


def test_two_input_files_reuse_the_parsed_reference_and_a_vcf_refuses_them(hip, bulk, tmp_path, monkeypatch):
    d, dbinfo, lines = bulk
    calls = []
    parse = _hip.Hip.refseq_from_file
    monkeypatch.setattr(_hip.Hip, "refseq_from_file", lambda self, *a, **k: calls.append(a[0]) or parse(self, *a, **k))
    so.VARIANTS._reference = None
    out = tmp_path / "two.tsv"
    args = sc.make_args(str(d / "b.sam"), dbinfo, str(tmp_path / "two.cami"), {"input_type": "AUTO", "ani": str(out),
                                                                              "reference": str(d / "ref.fa")})
    args.infiles = [str(d / "b.sam"), str(d / "b.bam")]
    mp.map_main(args)
    ani, _, _ = _definition(lines, dbinfo, d / "ref.fa")
    head, block = ani.split("\n", 2)[:2], ani.split("\n", 2)[2]
    assert out.read_text() == "\n".join(head) + "\n" + "".join("#file\t%s\n" % f + block for f in args.infiles)
    assert calls == [str(d / "ref.fa")]  # parsed once: both files have the same lengths
    args.vcf = str(tmp_path / "two.vcf")
    with pytest.raises(SystemExit) as e:
        mp.map_main(args)
    assert str(e.value.code) == so.VARIANTS.refuse_vcf_files
    for extra, text in (({"reference": "AUTO", "db": "NONE"}, so.VARIANTS.refuse_no_reference),
                        ({"reference": str(tmp_path / "none.fa")}, so.VARIANTS.refuse_reference_missing % (tmp_path / "none.fa"))):
        with pytest.raises(SystemExit) as e:
            mp.map_main(sc.make_args(str(d / "b.sam"), dbinfo, str(tmp_path / "r.cami"), dict({"ani": str(tmp_path / "r.tsv")}, **extra)))
        assert str(e.value.code) == text
