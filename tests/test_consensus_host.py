"""CPU: metalign_amd/consensus.py (the definition of --consensus) against a hand table, its flags and refusals, and the consensus
part of mg_variants_core.h — consensus_char, text_bytes, text_at — on the host under the sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import consensus_cases as cc
import variants_cases as vc
from metalign_amd import cli
from metalign_amd import consensus as con
from metalign_amd import coverage as cv
from metalign_amd import variants as var

HERE = os.path.dirname(os.path.abspath(__file__))
P = var.Params(5, 2, 50)
LOW = var.Params(2, 1, 0)


def _want_char(n4, p, ok, major, alleles, iupac):
    if not ok:
        return "N"
    return cc.IUPAC[(1 << major) | sum(1 << a for a in alleles)] if iupac else "ACGT"[major]


@pytest.mark.parametrize("n4, dcf, want", vc.SITE_CASES)
def test_the_site_character_over_the_site_rules_edges(n4, dcf, want):
    ok, major, alleles, _, _ = want
    p = var.Params(*dcf)
    for iupac in (False, True):
        assert con.char_of(n4, p, iupac) == _want_char(n4, p, ok, major, alleles, iupac)
    if ok and not alleles:  # a callable site that is not polymorphic: the same letter in both modes
        assert con.char_of(n4, p, True) == con.char_of(n4, p, False) == "ACGT"[major]


def test_all_fifteen_masks_depth_edge_and_ties():
    assert con.IUPAC == cc.IUPAC == "-ACMGRSVTWYHKDBN" and con.LINE_WIDTH == 60 and con.MODES == ("major", "iupac")
    got = {m: con.char_of(n4, LOW, True) for m, n4 in cc.MASK_CASES.items()}
    assert got == {m: cc.IUPAC[m] for m in range(1, 16)} and len(set(got.values())) == 15
    for m, n4 in cc.MASK_CASES.items():  # mode major: the lowest allele of the mask
        assert con.char_of(n4, LOW, False) == "ACGT"[(m & -m).bit_length() - 1]
    # d = D - 1 against d = D
    assert con.char_of([1, 0, 0, 0], LOW, True) == "N" and con.char_of([2, 0, 0, 0], LOW, True) == "A"
    assert con.char_of([1, 1, 1, 1], P, False) == "N" and con.char_of([1, 1, 1, 2], P, False) == "T"
    assert con.char_of([0, 0, 0, 0], LOW, False) == "N"  # only skip, or cover with other bytes
    # ties go to the lowest code
    assert [con.char_of(n4, LOW, False) for n4 in ([1, 1, 0, 0], [0, 1, 0, 1], [0, 0, 3, 3], [2, 2, 2, 2])] == ["A", "C", "G", "A"]
    assert [con.char_of(n4, LOW, True) for n4 in ([1, 1, 0, 0], [0, 1, 0, 1], [0, 0, 3, 3], [2, 2, 2, 2])] == ["M", "Y", "K", "N"]


@pytest.mark.parametrize("w", cc.TEXT_WIDTHS)
def test_the_text_of_a_sequence(w):
    for L in cc.text_lengths(w):
        seq = bytes(65 + i % 26 for i in range(L))
        text = con.text_of(seq, w)
        assert len(text) == con.text_bytes(L, w) == L + -(-L // w)
        assert text.replace(b"\n", b"") == seq and (text.endswith(b"\n") and not text.endswith(b"\n\n") if L else text == b"")
        assert all(len(ln) == w for ln in text.split(b"\n")[:-2]) and (not L or 1 <= len(text.split(b"\n")[-2]) <= w)
    assert con.text_of(b"ACGTA", 2) == b"AC\nGT\nA\n" and con.text_of(b"ACGT", 2) == b"AC\nGT\n" and con.text_of(b"", 60) == b""


def _records(p=P, iupac=False, min_called=0.0):
    return con.consensus(vc.HAND, vc.A2I, 0.5, p, iupac, min_called)


def test_hand_table_records():
    for (dcf, iupac), seqs in cc.HAND_SEQ.items():
        recs = _records(var.Params(*dcf), iupac)
        assert [r.acc for r in recs] == ["c1", "c2", "d1"]  # db_info order, the S rows of --variants
        for r in recs:
            assert r.seq == seqs[r.acc].encode() and len(r.seq) == r.length == cv.lengths_of([], vc.A2I)[r.acc]
            assert (r.alignments, r.called, r.ambiguous) == cc.HAND_CALLED[dcf][r.acc] and r.taxid == vc.A2I[r.acc][1]
        # called and ambiguous are the numbers --variants prints
        per = var.variants(vc.HAND, vc.A2I, 0.5, var.Params(*dcf)).per
        assert {r.acc: [r.alignments, r.called, r.ambiguous] for r in recs} == {a: st[:3] for a, st in per.items()}
    assert _records() == con.consensus(vc.HAND, vc.A2I, 0.5)  # (the defaults)


def test_exact_bytes_of_the_file_one_and_two_inputs_and_unique(tmp_path):
    path = str(tmp_path / "c.fa")
    con.write_consensus(path)
    assert open(path, "rb").read() == b""  # a new file is empty: no comment lines, no #reads line
    con.write_consensus(path, _records(), True, P, False)
    assert open(path, "rb").read() == cc.hand_file()
    con.write_consensus(path)
    for src in ("a.sam", "b.bam"):
        con.write_consensus(path, _records(), append=True, p=P, iupac=False, source=src)
    assert open(path, "rb").read() == cc.hand_file(" file=a.sam") + cc.hand_file(" file=b.bam")
    con.write_consensus(path)
    con.write_consensus(path, _records(), True, P, False, unique=True)
    assert open(path, "rb").read() == cc.hand_file(" reads=unique")
    con.write_consensus(path)
    con.write_consensus(path, _records(), True, P, False, unique=True, source="a.sam")
    assert open(path, "rb").read() == cc.hand_file(" reads=unique file=a.sam")
    con.write_consensus(path)
    con.write_consensus(path, _records(LOW, True), True, LOW, True)
    got = open(path, "rb").read().split(b"\n")
    assert got[0] == b">c1 taxid=g1.1 length=20 alignments=9 called=6 ambiguous=6 min_depth=2 min_count=1 min_freq_permille=0 ambiguity=iupac"
    assert got[1] == b"WHBBNKN" + b"N" * 13


def test_min_called_at_the_permille_edge():
    assert con.min_called_permille() == 0 and con.min_called_permille(1.0) == 1000 and con.min_called_permille(0.2) == 200
    assert con.min_called_permille(0.0125) == 12 and con.min_called_permille(0.0135) == 14  # int(round()), as variants.params
    for bad in (-0.001, 1.001, float("nan")):
        with pytest.raises(ValueError):
            con.min_called_permille(bad)
    # 1000 sites, 999 against 1000 of them callable
    a2i = {"Unmapped": [0, "Unmapped", "", ""], "k": [1000, "g", "", ""]}
    full = [vc.L("r%d" % i, 0, "k", 1, "1000M", "A" * 1000) for i in range(2)]
    short = [vc.L("r%d" % i, 0, "k", 1, "999M", "A" * 999) for i in range(2)]
    for lines, called in ((full, 1000), (short, 999)):
        recs = con.consensus(lines, a2i, 0.5, LOW, False, 0.0)
        assert [(r.called, r.length) for r in recs] == [(called, 1000)]
        assert len(con.consensus(lines, a2i, 0.5, LOW, False, 0.999)) == 1
        assert len(con.consensus(lines, a2i, 0.5, LOW, False, 1.0)) == (1 if called == 1000 else 0)
        assert len(con.consensus(lines, a2i, 0.5, LOW, False, 0.9996)) == (1 if called == 1000 else 0)  # M = 1000
        assert len(con.consensus(lines, a2i, 0.5, LOW, False, 0.9994)) == 1                              # M = 999
    assert con.written(1000, 999, 999) and not con.written(1000, 999, 1000) and con.written(0, 0, 1000)
    # the hand table: c1 has 4 of 20 callable (200 permille), c2 and d1 none
    assert [r.acc for r in _records(min_called=0.2)] == ["c1"] and _records(min_called=0.201) == []


def test_records_give_what_the_lines_give():
    from metalign_amd import _hip, map_and_profile as mp
    recs = mp.tokenise_sam(vc.HAND, vc.ACC_INDEX)
    entries, pool = var.entries_and_pool(f for f in map(cv.retained_fields, vc.HAND) if f is not None)
    names = ["Unmapped", "c1", "c2", "d1"]
    lengths = cv.lengths_of([], vc.A2I)
    for p, iupac in ((P, False), (LOW, True)):
        got = con.consensus_of_records(recs, np.array(entries, dtype=_hip.BASES_DTYPE), pool, names, lengths, 0.5, vc.A2I, p, iupac)
        assert got == _records(p, iupac) and len(got) == 3
    # ... and the span-1 records of consensus_cases give the counts they were made from
    counts = {1: {0: [5, 0, 0, 1], 3: [0, 1, 1, 2], 19: [0, 0, 1, 0]}, 3: {7: [2, 2, 2, 2]}}
    r, e, pl = cc.records_of_counts(counts)
    n, aln, unpiled = var.counts_of_records(r, e, pl, names, lengths, 0.5)
    assert n == {"c1": counts[1], "d1": counts[3]} and aln == {"c1": 6 + 4 + 1, "d1": 8} and unpiled == 0 and len(pl) == len(r) == 19


def test_slabs_of_consecutive_rows():
    assert con.SLAB_BYTES == 64 << 20
    assert con.slabs([]) == [] and con.slabs([5]) == [(0, 1)] and con.slabs([50, 50, 1], 100) == [(0, 2), (2, 3)]
    assert con.slabs([300, 10, 90, 1, 500, 500], 100) == [(0, 1), (1, 3), (3, 4), (4, 5), (5, 6)]  # a text longer than a slab is one
    assert con.slabs([0, 0, 0], 0) == [(0, 3)]


def test_the_flags_exist_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        assert acts["consensus"].default == "NONE" and acts["consensus"].option_strings == ["--consensus"]
        assert acts["consensus_ambiguity"].default == "major" and list(acts["consensus_ambiguity"].choices) == ["major", "iupac"]
        assert acts["consensus_min_called"].default == 0.0 and acts["consensus_min_called"].type is float
        pos = ["x.sam", "data"] if tool == "map_and_profile" else ["r.fq", "data"]
        args = cli.parser_for(tool).parse_args(pos + ["--consensus", "c.fa", "--consensus_ambiguity", "iupac", "--consensus_min_called", "0.5"])
        assert (args.consensus, args.consensus_ambiguity, args.consensus_min_called, args.variants) == ("c.fa", "iupac", 0.5, "NONE")
        args = cli.parser_for(tool).parse_args(pos)
        assert (args.consensus, args.consensus_ambiguity, args.consensus_min_called) == ("NONE", "major", 0.0)
        with pytest.raises(SystemExit):
            cli.parser_for(tool).parse_args(pos + ["--consensus_ambiguity", "both"])


def test_consensus_alone_opens_the_variants_family(tmp_path):
    import stage_c_checks as sc
    from metalign_amd import side_outputs as so
    assert so.FAMILIES == (so.COVERAGE, so.DEPTH, so.IDENTITY, so.VARIANTS) and so.VARIANTS.flags == ("variants", "variant_sites")
    fa = tmp_path / "c.fa"
    args = sc.make_args("x.sam", "db_info.txt", "o.cami", {"consensus": str(fa)})
    assert so.VARIANTS.wanted(args) and not any(f.wanted(args) for f in so.FAMILIES[:3]) and so.VARIANTS.paths(args) == []
    assert not so.VARIANTS.wanted(sc.make_args("x.sam", "db_info.txt", "o.cami", {}))
    sides = so.SideOutputs.of(args, "x.sam", header=lambda: ["@SQ\tSN:c1\tLN:7\n"])
    assert sides.families == (so.VARIANTS,) and sides.based and sides.sized and not sides.placed and not sides.edited
    # the estimate: what --variants holds, and a slab of text or all of it
    lengths = {"a": 1000, "b": 24}
    plain = so.SideOutputs.of(sc.make_args("x.sam", "db_info.txt", "o.cami", {"variants": "v.tsv"}), "x.sam")
    assert plain.need_bytes(lengths, 2, 10) == 16 * 1024 + 40 * 2 + 96 * 10
    assert sides.need_bytes(lengths, 2, 10) == plain.need_bytes(lengths, 2, 10) + (1000 + 17) + (24 + 1)
    big = {"a": 200 << 20}
    assert sides.need_bytes(big, 1, 0) == plain.need_bytes(big, 1, 0) + con.SLAB_BYTES
    # the header: an empty file, and no #reads line under --side_reads unique either
    so.write_headers(args)
    assert fa.read_bytes() == b""
    args.side_reads = "unique"
    so.check_flags(args)  # (--consensus is one of the outputs --side_reads unique needs)
    so.write_headers(args)
    assert fa.read_bytes() == b""
    # a collated input's records come from the definition, with and without the TSV beside them
    for extra, unique in (({}, False), ({"variants": str(tmp_path / "v.tsv")}, False), ({"side_reads": "unique"}, True)):
        a = sc.make_args("x.sam", "db_info.txt", "o.cami", dict({"consensus": str(fa)}, **extra))
        so.write_headers(a)
        so.SideOutputs.of(a, "x.sam").append_from_definition("x.sam", lambda: iter(vc.HAND), vc.A2I, vc.T2I)
        assert fa.read_bytes() == cc.hand_file(" reads=unique" if unique else "")
        if "variants" in extra:
            assert (tmp_path / "v.tsv").read_text() == vc.HAND_FILE


def test_the_driver_writes_slab_by_slab_and_halves_a_slab_that_has_no_room(tmp_path):
    """_Variants.close over a stand-in for the accumulator: the rows that are written, the slabs, the halving on ERR_NOMEM down to
    one row, and the accumulator freed on every way out."""
    import stage_c_checks as sc
    from metalign_amd import _hip, side_outputs as so
    seqs = {vc.ACC_INDEX[r.acc]: con.text_of(r.seq) for r in _records()}

    class Dev:
        def __init__(self, room):
            self.room, self.calls, self.freed = room, [], 0

        def result(self, *p):
            assert p == tuple(P)
            u = lambda xs: np.array(xs, dtype=np.uint64)
            return u([0, 9, 1, 1]), u([0, 4, 0, 0]), u([0, 1, 0, 0]), u([0, 122, 0, 0]), u([0, 72, 0, 0]), 6, np.zeros(0, _hip.VARIANT_SITE_DTYPE)

        def consensus(self, rows, D, C, F, iupac, width=60):
            assert not self.freed and (D, C, F, iupac, width) == (5, 2, 50, False, 60)
            self.calls.append(list(rows))
            if len(rows) > self.room:
                raise _hip.HipError("no room", _hip.ERR_NOMEM if self.room >= 0 else _hip.ERR_HIP)
            return b"".join(seqs[r] for r in rows)

        def free(self):
            self.freed += 1

    fa = tmp_path / "c.fa"
    lengths = cv.lengths_of([], vc.A2I)

    def close(dev, **extra):
        args = sc.make_args("x.sam", "db_info.txt", "o.cami", dict({"consensus": str(fa)}, **extra))
        so.write_headers(args)
        so.VARIANTS.close(args, "x.sam", lengths, dev, vc.ACC_INDEX, vc.A2I, vc.T2I)

    dev = Dev(room=3)
    close(dev)
    assert fa.read_bytes() == cc.hand_file() and dev.calls == [[1, 2, 3]] and dev.freed == 1
    dev = Dev(room=1)
    close(dev)
    assert fa.read_bytes() == cc.hand_file() and dev.calls == [[1, 2, 3], [1], [2, 3], [2], [3]] and dev.freed == 1
    dev = Dev(room=3)
    close(dev, consensus_min_called=0.2, variants=str(tmp_path / "v.tsv"))
    assert fa.read_bytes() == cc.hand_file().split(b">c2")[0] and dev.calls == [[1]] and (tmp_path / "v.tsv").read_text() == vc.HAND_FILE
    for room in (0, -1):  # one row does not fit; another error: raised, and the accumulator freed all the same
        dev = Dev(room)
        with pytest.raises(_hip.HipError) as e:
            close(dev)
        assert e.value.code == (_hip.ERR_NOMEM if room == 0 else _hip.ERR_HIP) and dev.freed == 1 and dev.calls == ([[1, 2, 3], [1]] if room == 0 else [[1, 2, 3]])


def test_map_main_refuses_two_processes_paf_and_min_called_out_of_range(monkeypatch, tmp_path):
    import stage_c_checks as sc
    from metalign_amd import _hip, map_and_profile as mp, select_db

    def never(*a, **k):
        raise AssertionError("refused before the process group, the GPU or the library is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    out = tmp_path / "consensus.fa"

    def refused(infile, extra):
        args = sc.make_args(str(tmp_path / infile), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)
        with pytest.raises(SystemExit) as e:
            mp.map_main(args)
        assert "\n" not in str(e.value.code) and not out.exists()
        return str(e.value.code)

    paf = "Error: --consensus needs SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns."
    assert refused("x.paf", {"consensus": str(out), "input_type": "AUTO"}) == paf
    assert refused("x.sam", {"consensus": str(out), "paf_input": True}) == paf
    # with a --variants flag present the existing message stands
    assert refused("x.paf", {"consensus": str(out), "variants": str(tmp_path / "v.tsv"), "input_type": "AUTO"}) == (
        "Error: --variants and --variant_sites need SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.")
    for bad in (-0.01, 1.01):
        assert refused("x.sam", {"consensus": str(out), "consensus_min_called": bad}) == "Error: --consensus_min_called must lie within 0 to 1."
    assert refused("x.sam", {"consensus": str(out), "variant_min_depth": 1}) == "Error: --variant_min_depth must be at least 2."
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert refused("x.sam", {"consensus": str(out)}) == ("Error: --consensus runs in one process on one GPU; start it without "
                                                        "torch.distributed.run.")
    assert refused("x.sam", {"consensus": str(out), "variant_sites": str(tmp_path / "s.tsv")}) == (
        "Error: --variants and --variant_sites run in one process on one GPU; start it without torch.distributed.run.")


# ---- mg_variants_core.h on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("consensus") / "host_consensus_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_consensus_check.cpp")])
    return out


def test_core_header_character_and_text_layout(exe, tmp_path):
    chars = []
    table = [(n4, dcf) for n4, dcf, _ in vc.SITE_CASES] + [(n4, (2, 1, 0)) for n4 in cc.PATTERNS]
    table += [(n4, tuple(P)) for n4 in vc.HAND_COUNTS["c1"].values()] + [([2 ** 32 - 1, 2 ** 32 - 1, 0, 2 ** 31], (5, 2, 500))]
    for n4, dcf in table:
        for iupac in (0, 1):
            chars.append(struct.pack("<9I", *n4, *dcf, iupac, ord(con.char_of(n4, var.Params(*dcf), bool(iupac)))))
    texts = []
    pairs = [(L, w) for w in cc.TEXT_WIDTHS for L in cc.text_lengths(w)] + [(L, w) for w in cc.WIDTHS for L in cc.LENGTHS[:-1]]
    pairs += [(L, cc.ROW_WIDTH) for L in cc.ROW_LENGTHS] + [(cc.LENGTHS[-1], 60), (65535, 65535), (65536, 65535)]
    for L, w in pairs:
        seq = bytes(65 + (i * 7 + i // 26) % 26 for i in range(L))
        text = con.text_of(seq, w)
        texts.append(struct.pack("<QIQ", L, w, len(text)) + seq + text)
    p = tmp_path / "cases.bin"
    p.write_bytes(struct.pack("<I", len(chars)) + b"".join(chars) + struct.pack("<I", len(texts)) + b"".join(texts))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.decode().splitlines()[-1] == "%d characters, %d texts, 0 differ" % (len(chars), len(texts))
    assert len(chars) > 80 and len(texts) > 70
