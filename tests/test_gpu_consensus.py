"""-m gpu: --consensus on the device — mg_variants_consensus (mg_variants.hip: k_var_consensus), its binding and the command line.
The expectation is always metalign_amd/consensus.py over the same records / lines, and every comparison is byte for byte."""
import functools
import gzip

import numpy as np
import pytest

import bamgen
import collate_cases
import consensus_cases as cc
import identity_cases as ic
import stage_c_checks as sc
import variants_cases as vc
from metalign_amd import _hip
from metalign_amd import collate
from metalign_amd import consensus as con
from metalign_amd import map_and_profile as mp
from metalign_amd import side_reads as sr
from metalign_amd import variants as var

pytestmark = pytest.mark.gpu

PCT = 0.5
P = var.Params(5, 2, 50)
LOW = var.Params(2, 1, 0)
GUARD = 0xA5


def _seqs(names, lengths, recs, ent, pool, p):
    """The definition over the records: {iupac: [the sequence of every row]}; a row without an alignment is N throughout."""
    len_of = dict(zip(names, lengths))
    n, aln, unpiled = var.counts_of_records(recs, ent, pool, names, len_of, PCT)
    a2i = {a: [L, "t"] for a, L in len_of.items()}
    out = {}
    for iupac in (False, True):
        got = {r.acc: r.seq for r in con.records_of(n, aln, unpiled, len_of, names, a2i, p, iupac)}
        assert set(got) == {a for a in names if aln.get(a)}
        out[iupac] = [got.get(a, b"N" * len_of[a]) for a in names]
    return out


def _fetch(dev, rows, p, iupac, width):
    """The texts of `rows` into an array with guard bytes behind them, which stay."""
    n = dev.text_bytes(rows, width)
    out = np.full(n + 64, GUARD, dtype=np.uint8)
    dev.consensus_into(rows, p.min_depth, p.min_count, p.permille, iupac, width, out, n)
    assert (out[n:] == GUARD).all()
    return out[:n].tobytes()


def _want(seqs, rows, width):
    return b"".join(con.text_of(seqs[r], width) for r in rows)


class _Case:
    def __init__(self, hip, lengths, quiet=(), p=LOW):
        self.names = ["a%d" % i for i in range(len(lengths))]
        self.lengths, self.p = list(lengths), p
        recs, ent, pool = cc.records_of_counts(cc.pattern_counts(lengths, quiet))
        self.seqs = _seqs(self.names, lengths, recs, ent, pool, p)
        self.dev = hip.variants(lengths)
        try:
            self.dev.add(recs, ent, pool, PCT)
        except BaseException:
            self.dev.free()
            raise

    def check(self, rows, width, modes=(False, True)):
        for iupac in modes:
            assert _fetch(self.dev, rows, self.p, iupac, width) == _want(self.seqs[iupac], rows, width), (rows, width, iupac)


@pytest.fixture(scope="module")
def in_a_row(hip):
    case = _Case(hip, cc.ROW_LENGTHS)
    yield case
    case.dev.free()


@pytest.fixture(scope="module")
def layout(hip):
    """cc.LENGTHS and behind them an accession nobody hits."""
    case = _Case(hip, cc.LENGTHS + [131], quiet=(len(cc.LENGTHS),))
    yield case
    case.dev.free()


def test_lengths_1_to_17_in_a_row_at_width_5(in_a_row):
    """Every text starts at another residue mod 4 and mod 16, newlines fall in every byte of a store word."""
    rows = list(range(len(cc.ROW_LENGTHS)))
    starts = np.cumsum([0] + [con.text_bytes(L, cc.ROW_WIDTH) for L in cc.ROW_LENGTHS])[:-1]
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3} and len({int(s) % 16 for s in starts}) >= 10
    want = _want(in_a_row.seqs[True], rows, cc.ROW_WIDTH)
    assert {i % 4 for i, b in enumerate(want) if b == 10} == {0, 1, 2, 3} and len(set(want)) > 12
    in_a_row.check(rows, cc.ROW_WIDTH)
    in_a_row.check(rows[::-1], cc.ROW_WIDTH)
    for r in rows:  # every row alone: the buffer's last word is partial in most of them
        in_a_row.check([r], cc.ROW_WIDTH, modes=(True,))


@pytest.mark.parametrize("width", cc.WIDTHS)
def test_lengths_around_a_line_a_step_and_many_workgroups(layout, width):
    nrows = len(layout.lengths)
    assert cc.LENGTHS == [0, 59, 60, 61, 120, 121, 4096, 4097, 70001] and nrows == 10
    assert layout.seqs[False][9] == b"N" * 131 and len(set(layout.seqs[True][8])) >= 15
    layout.check(list(range(nrows)), width)
    layout.check(list(range(nrows))[::-1], width, modes=(True,))
    layout.check([7, 3, 9, 7, 0, 1, 7], width, modes=(True,))  # a subset with a repeat, the quiet row and the empty one among them
    layout.check([9], width, modes=(False,))                   # a row without any alignment: all N
    layout.check([0], width, modes=(False,))                   # a row without a base: no byte
    layout.check([], width, modes=(False,))                    # nrows = 0


def test_the_binding_returns_the_same_bytes(layout):
    rows = [5, 2, 8]
    got = layout.dev.consensus(rows, *LOW, True)
    assert isinstance(got, bytes) and got == _want(layout.seqs[True], rows, 60) == _fetch(layout.dev, rows, LOW, True, 60)
    assert layout.dev.consensus([], *LOW, False, width=7) == b"" and layout.dev.consensus([0, 0], *LOW, False) == b""


@pytest.mark.parametrize("width", [3, 60])
def test_the_grid_cut_to_a_few_workgroups(layout, width):
    rows = list(range(len(layout.lengths)))
    full = _fetch(layout.dev, rows, LOW, True, width)
    for grid in (1, 2):
        _hip.debug_set("var_grid", grid)
        try:
            assert _hip.debug_get("var_grid") == grid
            cut = _fetch(layout.dev, rows, LOW, True, width)
        finally:
            _hip.debug_set("var_grid", 0)
        assert cut == full
    assert full == _want(layout.seqs[True], rows, width)


def test_both_modes_over_the_fifteen_masks_and_the_threshold_edges(hip):
    """Site i of one accession holds the i-th of SITE_CASES' and MASK_CASES' counts; every parameter set judges all of them."""
    table = [n4 for n4, _, _ in vc.SITE_CASES] + list(cc.MASK_CASES.values())
    recs, ent, pool = cc.records_of_counts({0: dict(enumerate(table))})
    params = sorted({var.Params(*dcf) for _, dcf, _ in vc.SITE_CASES} | {LOW})
    dev = hip.variants([len(table)])
    try:
        dev.add(recs, ent, pool, PCT)
        for p in params:
            for iupac in (False, True):
                want = "".join(con.char_of(n4, p, iupac) for n4 in table)
                assert _fetch(dev, [0], p, iupac, 60) == want.encode() + b"\n", (p, iupac)
        masks = _fetch(dev, [0], LOW, True, 60)[len(vc.SITE_CASES):-1]
        assert masks == cc.IUPAC[1:].encode()  # all fifteen, in the order of the masks
        for n4, dcf, (ok, major, alleles, _, _) in vc.SITE_CASES:  # (the table's own expectations, not only char_of's)
            i, p = [t for t, _, _ in vc.SITE_CASES].index(n4), var.Params(*dcf)
            both = _fetch(dev, [0], p, False, 60)[i:i + 1], _fetch(dev, [0], p, True, 60)[i:i + 1]
            mask = (1 << major) | sum(1 << a for a in alleles)
            assert both == ((b"ACGT"[major:major + 1], cc.IUPAC[mask].encode()) if ok else (b"N", b"N")), (n4, dcf)
    finally:
        dev.free()
    assert len(params) >= 6


def test_before_a_finish_between_finish_and_fetch_and_after_a_further_add(hip):
    names, lengths = ["x", "y"], [70, 9]
    first = {0: {3: [3, 0, 0, 0], 4: [2, 1, 0, 0], 69: [0, 0, 2, 2]}, 1: {0: [0, 2, 0, 0]}}
    more = {0: {3: [0, 4, 0, 0], 5: [0, 0, 0, 2]}, 1: {8: [1, 1, 1, 1]}}
    a, b = cc.records_of_counts(first), cc.records_of_counts(more)
    both = (np.concatenate([a[0], b[0]]), np.concatenate([a[1], np.array([(o + len(a[2]), p, s) for o, p, s in b[1].tolist()],
                                                                         dtype=_hip.BASES_DTYPE)]), a[2] + b[2])
    want1, want2 = _seqs(names, lengths, *a, LOW), _seqs(names, lengths, *both, LOW)
    assert want1[True][0][3:6] == b"AMN" and want2[True][0][3:6] == b"MMT" and want2[True][1] == b"C" + b"N" * 8
    dev = hip.variants(lengths)
    try:
        assert _fetch(dev, [0, 1], LOW, True, 60) == _want([b"N" * 70, b"N" * 9], [0, 1], 60)  # the zeros of create
        dev.add(*a, PCT)
        assert _fetch(dev, [0, 1], LOW, True, 60) == _want(want1[True], [0, 1], 60)  # before any finish
        res = dev.finish(*LOW)
        sites = dev.fetch_sites()
        assert res[6] == len(sites) == 2
        assert _fetch(dev, [1, 0], LOW, False, 7) == _want(want1[False], [1, 0], 7)
        again = dev.fetch_sites()  # still the last finish's sites
        assert np.array_equal(again, sites) and [(int(s["acc"]), int(s["pos0"])) for s in again] == [(0, 4), (0, 69)]
        dev.add(*b, PCT)
        assert _fetch(dev, [0, 1], LOW, True, 60) == _want(want2[True], [0, 1], 60)  # the new counts
        assert np.array_equal(dev.fetch_sites(), sites)  # (and no finish since)
        assert dev.finish(*LOW)[6] == 4  # (sites 3, 4 and 69 of x, site 8 of y)
    finally:
        dev.free()


def test_arguments_out_of_range_are_refused(layout):
    dev, n = layout.dev, len(layout.lengths)
    size = dev.text_bytes([1, 2], 60)
    out = np.full(size + 64, GUARD, dtype=np.uint8)

    def refused(rows, p, iupac, width, nbytes):
        with pytest.raises(_hip.HipError) as e:
            dev.consensus_into(rows, *p, iupac, width, out, nbytes)
        assert e.value.code == _hip.ERR_ARG and (out == GUARD).all()
        return str(e.value)

    assert "%d" % n in refused([1, n], LOW, 0, 60, size)  # row = nacc
    refused([1, 2], LOW, 0, 0, size)
    refused([1, 2], LOW, 0, 65536, size)
    refused([1, 2], LOW, 2, 60, size)
    assert str(size) in refused([1, 2], LOW, 0, 60, size - 1) and str(size) in refused([1, 2], LOW, 0, 60, size + 1)
    assert " 0 bytes" in refused([], LOW, 0, 60, 1)
    for bad in ((1, 2, 50), (5, 0, 50), (5, 2, 501)):
        refused([1, 2], var.Params(*bad), 0, 60, size)
    dev.consensus_into([1, 2], *LOW, 0, 65535, out, dev.text_bytes([1, 2], 65535))  # the widest line
    assert out[:62].tobytes() == _want(layout.seqs[False], [1], 65535) + layout.seqs[False][2][:2] and (out[size:] == GUARD).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _definition(lines, dbinfo, p=P, iupac=False, min_called=0.0, unique=False, source=None):
    args = sc.make_args("x.sam", dbinfo, "-", {})
    acc2info, _ = mp.get_acc2info(args)
    if unique:
        lines = sr.unique_lines(lines, acc2info, PCT)
    recs = con.consensus(lines, acc2info, PCT, p, iupac, min_called)
    return b"".join(con.format_record(r, p, iupac, unique, source) for r in recs), recs


def _run(path, dbinfo, tmp_path, tag, **extra):
    (tmp_path / tag).mkdir()
    fa, out = tmp_path / tag / "consensus.fa", tmp_path / tag / "out.cami"
    mp.map_main(sc.make_args(str(path), dbinfo, str(out), dict({"input_type": "sam", "db": "unused.fna", "sampleID": "s",
                                                                "consensus": str(fa)}, **extra)))
    return fa.read_bytes(), out.read_bytes()


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("consensus_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = vc.dress(ic.dress(open(sam).read(), 52), 53)
    text = "".join(lines)
    (d / "b.sam").write_text(text)
    (d / "b.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "b.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    return d, [d / "b.sam", d / "b.sam.gz", d / "b.bam"], dbinfo, lines, _definition(lines, dbinfo)


def test_map_main_sam_gz_and_bam_give_the_definitions_bytes(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, (want, recs) = bulk
    assert len(recs) > 10 and sum(r.called for r in recs) > 200 and sum(r.ambiguous for r in recs) > 20
    assert want.count(b">") == len(recs) and all(len(ln) <= 60 for ln in want.split(b"\n") if not ln.startswith(b">"))
    cami0 = None
    for path in forms:  # --consensus alone
        got, cami = _run(path, dbinfo, tmp_path, "alone_" + path.name)
        assert got == want and cami == (cami0 or cami), path.name
        cami0 = cami
    v0 = tmp_path / "v0.tsv"
    mp.map_main(sc.make_args(str(forms[0]), dbinfo, str(tmp_path / "v0.cami"), {"input_type": "sam", "db": "unused.fna", "sampleID": "s",
                                                                                "variants": str(v0)}))
    assert (tmp_path / "v0.cami").read_bytes() == cami0
    # with --variants alongside: the TSV is what it is without --consensus, and every header's called / ambiguous are its columns
    v = tmp_path / "v.tsv"
    got, _ = _run(forms[2], dbinfo, tmp_path, "with_variants", variants=str(v))
    assert got == want and v.read_bytes() == v0.read_bytes()
    tsv = {f[1]: (f[4], f[5], f[6]) for f in (ln.split("\t") for ln in v.read_text().splitlines()) if f[0] == "S"}
    heads = [dict(kv.split("=") for kv in ln.split()[1:]) | {"acc": ln.split()[0][1:]} for ln in got.decode().splitlines() if ln.startswith(">")]
    assert {h["acc"]: (h["alignments"], h["called"], h["ambiguous"]) for h in heads} == tsv and len(tsv) == len(recs)


def test_map_main_iupac_min_called_and_other_thresholds(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, (want, recs) = bulk
    want_i, _ = _definition(lines, dbinfo, iupac=True)
    assert want_i != want and _run(forms[0], dbinfo, tmp_path, "iupac", consensus_ambiguity="iupac")[0] == want_i
    share = sorted(1000 * r.called // r.length for r in recs)
    cut = (share[len(share) // 2] + 1) / 1000.0  # drops about half of the accessions
    want_c, kept = _definition(lines, dbinfo, min_called=cut)
    assert 0 < len(kept) < len(recs)
    assert _run(forms[2], dbinfo, tmp_path, "min_called", consensus_min_called=cut)[0] == want_c
    assert _run(forms[0], dbinfo, tmp_path, "none_called", consensus_min_called=1.0)[0] == b""
    other = dict(variant_min_depth=3, variant_min_count=1, variant_min_freq=0.2)
    want_o, _ = _definition(lines, dbinfo, p=var.params(3, 1, 0.2), iupac=True)
    assert _run(forms[1], dbinfo, tmp_path, "other", consensus_ambiguity="iupac", **other)[0] == want_o


def test_map_main_unique_reads_and_a_coordinate_sorted_copy(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, (want, _) = bulk
    want_u, _ = _definition(lines, dbinfo, unique=True)
    assert want_u != want and b" reads=unique\n" in want_u
    assert _run(forms[0], dbinfo, tmp_path, "unique", side_reads="unique")[0] == want_u
    shuffled = collate_cases.coordinate_shuffle("".join(lines))
    text = "".join(shuffled)
    (tmp_path / "s.sam").write_text(text)
    (tmp_path / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    want_s, _ = _definition(shuffled, dbinfo)
    want_su, _ = _definition(list(collate.collated_lines(shuffled)), dbinfo, unique=True)
    for name in ("s.sam", "s.bam"):
        assert _run(tmp_path / name, dbinfo, tmp_path, "sorted_" + name, collate="always")[0] == want_s, name
    assert _run(tmp_path / "s.sam", dbinfo, tmp_path, "sorted_unique", collate="always", side_reads="unique")[0] == want_su


def test_two_input_files_give_records_tagged_with_their_file(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, _ = bulk
    fa = tmp_path / "two.fa"
    args = sc.make_args(str(forms[0]), dbinfo, str(tmp_path / "two.cami"), {"input_type": "AUTO", "consensus": str(fa)})
    args.infiles = [str(forms[0]), str(forms[2])]
    mp.map_main(args)
    want = b"".join(_definition(lines, dbinfo, source=src)[0] for src in args.infiles)
    assert fa.read_bytes() == want and want.count((" file=%s\n" % forms[2]).encode()) > 10


@pytest.mark.parametrize("slab", [100, 120000])
def test_several_slabs_and_a_row_longer_than_a_slab(hip, bulk, tmp_path, monkeypatch, slab):
    d, forms, dbinfo, lines, (want, recs) = bulk
    sizes = [con.text_bytes(r.length) for r in recs]
    assert len(con.slabs(sizes, slab)) > 3 and max(sizes) > 100 and (slab == 100 or any(e - f > 1 for f, e in con.slabs(sizes, slab)))
    calls = []
    fetch = _hip.VariantsAcc.consensus
    monkeypatch.setattr(con, "SLAB_BYTES", slab)
    monkeypatch.setattr(_hip.VariantsAcc, "consensus", lambda self, rows, *a, **k: calls.append(len(rows)) or fetch(self, rows, *a, **k))
    assert _run(forms[0], dbinfo, tmp_path, "slabs")[0] == want
    assert calls == [e - f for f, e in con.slabs(sizes, slab)]
