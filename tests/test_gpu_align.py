"""-m gpu: the seed-and-extend aligner on the device (mg_align.hip) against its definition (metalign_amd/align.py) — the index, the
records with their places, edits and bases at every case of tests/align_cases.py, every batch size and a few workgroups, the
planted reads, and --aligner device through map_main and metalign.main against the same runs on the definition's SAM text."""
import gzip
import os

import numpy as np
import pytest

import align_cases as ac
import stage_c_checks as sc
from metalign_amd import _hip, align, refseq
from metalign_amd import map_and_profile as mp

pytestmark = pytest.mark.gpu


def parse_reference(hip, fasta, names, lengths, shift=0):
    """The FASTA text `shift` bytes behind a 16-byte boundary of a device buffer -> RefSeq."""
    text = np.frombuffer(b"\n" * shift + fasta, dtype=np.uint8)
    dev, index = hip.array(text if text.size else np.zeros(1, np.uint8)), hip.acc_index(list(names))
    try:
        return hip.refseq_parse(dev.ptr + shift, len(fasta), index, np.asarray(lengths, dtype=np.uint64))
    finally:
        dev.free()
        index.free()


class OnDevice:
    """A case table's reference and index on the device."""

    def __init__(self, hip, t, shift=0):
        self.hip, self.t = hip, t
        self.ref = parse_reference(hip, t.fasta, t.names, t.lengths, shift)
        self.index = hip.align_index(self.ref, t.p.k, t.p.w)

    def align(self, seqs, p=None, **want):
        bases, offs = ac.packed(seqs)
        d_b, d_o = self.hip.array(bases if bases.size else np.zeros(8, np.uint8)), self.hip.array(offs)
        try:
            return self.hip.align_reads_dev(self.index, d_b.ptr, d_o.ptr, len(seqs), p or self.t.p, **want)
        finally:
            d_b.free()
            d_o.free()

    def free(self):
        self.index.free()
        self.ref.free()


@pytest.fixture(scope="module", params=ac.PARAMS, ids=lambda kw: "k%d_w%d" % kw)
def dev(hip, request):
    d = OnDevice(hip, ac.table(*request.param))
    yield d
    d.free()


def check_batch(batch, stats, seqs, alns, want_stats, placed=True, edited=True, based=True, case=""):
    recs, places, edits, entries, pool = align.records(seqs, alns)
    assert stats == want_stats, (case, stats, want_stats)
    assert batch.count == len(recs) and np.array_equal(batch.download(), recs), case
    if placed:
        assert np.array_equal(batch.places(), places), case
    if edited:
        assert np.array_equal(batch.edits(), edits), case
    if based:
        got_entries, got_pool = batch.bases()
        assert np.array_equal(got_entries, entries) and got_pool == pool, case


# ---- the index ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 5])
def test_the_index_entries_equal_the_definitions(hip, dev, shift):
    """Every genome of the generator — the row without a reference, the copy, the repeats, N runs and lower case among them — at
    this (k, w); the reference text at two offsets from a 16-byte boundary."""
    t = dev.t
    d = dev if shift == 0 else OnDevice(hip, t, shift)
    try:
        assert d.ref.loaded().tolist() == t.ref.loaded
        entries = d.index.download()
        assert entries == t.entries and len(entries) > 1000
        assert d.index.stats() == (len(entries), len({e[0] for e in entries}), t.p.k, t.p.w)
    finally:
        if d is not dev:
            d.free()


def test_an_empty_reference_and_one_without_any_record(hip):
    for fasta, names, lengths in ((b"", [], []), (b"", ["a", "b"], [40, 0]), (b">a\nACGT\n", ["a"], [4])):
        ref = parse_reference(hip, fasta, names, lengths)
        index = hip.align_index(ref, 15, 5)
        try:
            assert index.download() == [] and index.stats()[:2] == (0, 0)
            bases, offs = ac.packed([b"ACGT" * 40, b""])
            d_b, d_o = hip.array(bases), hip.array(offs)
            batch, stats = hip.align_reads_dev(index, d_b.ptr, d_o.ptr, 2, align.params(), placed=True, edited=True, based=True)
            assert batch.count == 0 and stats == (2, 0, 0, 0, 0)
            batch.free()
            d_b.free()
            d_o.free()
        finally:
            index.free()
            ref.free()


def test_index_arguments_out_of_range_are_refused(hip, dev):
    for k, w in ((10, 5), (16, 5), (33, 5), (15, 0), (15, 33)):
        with pytest.raises(_hip.HipError) as e:
            hip.align_index(dev.ref, k, w)
        assert e.value.code == _hip.ERR_ARG
    bases, offs = ac.packed([b"ACGT" * 10])
    d_b, d_o = hip.array(bases), hip.array(offs)
    try:
        for bad in (dev.t.p._replace(k=dev.t.p.k + 2), dev.t.p._replace(min_score=0), dev.t.p._replace(max_secondary=16)):
            with pytest.raises(_hip.HipError) as e:
                hip.align_reads_dev(dev.index, d_b.ptr, d_o.ptr, 1, bad)
            assert e.value.code == _hip.ERR_ARG
    finally:
        d_b.free()
        d_o.free()


def test_an_index_that_cannot_fit_is_refused_by_arithmetic(hip):
    """Lengths whose minimizers alone (w = 1: every position, 48 bytes each) exceed the device's free memory: MG_ERR_NOMEM naming
    the bytes, before anything of the index is allocated or launched.  The reference rows hold no record: nothing is read."""
    free, _, pooled = hip.mem_info()
    n = (free + pooled) // 40
    ref = parse_reference(hip, b"", ["huge"], [n])
    hip.prof_enable(True)
    hip.prof_reset()
    try:
        with pytest.raises(_hip.HipError) as e:
            hip.align_index(ref, 11, 1)
        assert e.value.code == _hip.ERR_NOMEM and str(48 * (n - 10)) in str(e.value), e.value
        assert hip.prof_get("align_index")[0] == 0  # (the build's timed region, kernels and sorts, was never entered)
    finally:
        hip.prof_enable(False)
        ref.free()
    hip.mem_trim()


# ---- the alignment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1, 2])
def test_every_case_at_every_batch_size(dev, knobs, grid):
    """The whole case table: stats, records, places, edits, base entries and pool equal the definition's, on the launcher's grid
    and with seeding, extension and selection cut to 1 and 2 workgroups."""
    knobs("align_grid", grid)
    for n in ac.BATCH_SIZES + [len(dev.t.reads)]:
        names, seqs, alns, want = ac.batch_of(dev.t, n)
        batch, stats = dev.align(seqs, placed=True, edited=True, based=True)
        try:
            check_batch(batch, stats, seqs, alns, want, case="n=%d grid=%d" % (n, grid))
        finally:
            batch.free()
    # (the table is no empty check; at k = 31 every candidate is accepted, at the smaller k chance seeds are not)
    assert want.aligned > 30 and want.records > want.aligned and want.candidates >= want.accepted > want.records


def test_the_case_table_holds_what_it_promises(dev):
    t = dev.t
    kept = t.alns
    assert len(kept["duplicated"]) == 2 and {x.a for x in kept["duplicated"]} == {t.names.index("len5000"), t.names.index("copy")}
    assert all(x.a != t.names.index("absent") for v in kept.values() for x in v)
    for name in ("across", "across_rc"):  # never across the boundary of two accessions
        for x in kept[name]:
            assert 0 <= x.d + x.b and x.d + x.e <= t.lengths[x.a]
    assert len({(x.a, x.strand) for x in kept["tie"]}) == 2 and len({x.score for x in kept["tie"]}) == 1 and len(kept["tie"]) == 3
    assert t.stats_of["tandem"][1] > len(kept["tandem"]) >= 1  # overlapping diagonals collapsed
    assert kept["fwd1025"] == [] and kept["fwd0"] == [] and kept["all_n"] == []
    assert kept["left1"][0].d == -1 and kept["left1"][0].b == 1


@pytest.mark.parametrize("want", [dict(), dict(placed=True), dict(edited=True), dict(based=True), dict(placed=True, edited=True, based=True)],
                         ids=["none", "places", "edits", "bases", "all"])
def test_every_subset_of_the_side_arrays_gives_the_same_records(dev, want):
    names, seqs, alns, stats_want = ac.batch_of(dev.t, len(dev.t.reads))
    batch, stats = dev.align(seqs, **want)
    try:
        check_batch(batch, stats, seqs, alns, stats_want, placed=want.get("placed", False), edited=want.get("edited", False),
                    based=want.get("based", False), case=str(want))
        for side, fetch in (("placed", batch.places), ("edited", batch.edits), ("based", batch.bases)):
            if not want.get(side):
                with pytest.raises(_hip.HipError) as e:
                    fetch()
                assert e.value.code == _hip.ERR_STATE
    finally:
        batch.free()


def test_batches_appended_and_halved_give_one_batch(dev, knobs):
    """Three calls into one batch, and a candidate budget so small that the library halves every range of reads down to single
    reads: the records of the reads, in file order, as one call gives them."""
    names, seqs, alns, want = ac.batch_of(dev.t, len(dev.t.reads))
    cuts = [0, 7, 40, len(seqs)]
    batch, total = None, np.zeros(5, dtype=np.int64)
    for lo, hi in zip(cuts, cuts[1:]):
        batch, stats = dev.align(seqs[lo:hi], placed=True, edited=True, based=True, batch=batch)
        total += np.asarray(stats)
    try:
        check_batch(batch, align.Stats(*total.tolist()), seqs, alns, want, case="appended")
    finally:
        batch.free()
    t = dev.t

    def raw(seq):  # the candidates a read emits before they are made distinct: one per entry of every minimizer that seeds
        L = len(seq)
        if L < t.p.k or L > align.MAX_READ:
            return 0
        occ = [len(t.index.get(key, ())) for key, _, _ in align.minimizers(refseq.codes_of(seq), t.p.k, t.p.w)]
        return sum(n for n in occ if n <= t.p.max_occ)

    most = max(raw(s) for s in set(seqs))
    assert most > 20
    knobs("align_batch_cands", most)  # (the budget of a range of reads: what the hungriest single read needs)
    batch, stats = dev.align(seqs, placed=True, edited=True, based=True)
    try:
        check_batch(batch, stats, seqs, alns, want, case="halved")
    finally:
        batch.free()


def test_other_parameters(dev):
    """max_occ 1, no secondaries, a secondary share of 0 and 100 %, mismatch 1 and a min_score above every read's."""
    t = dev.t
    seqs = [s for _, s in t.reads]
    for change in (dict(max_occ=1), dict(max_secondary=0), dict(sec_pct=0, max_secondary=15), dict(sec_pct=100), dict(mismatch=1),
                   dict(min_score=1024), dict(min_score=1)):
        p = t.p._replace(**change)
        alns, want = align.align_reads(seqs, t.ref, p, index=t.index)
        batch, stats = dev.align(seqs, p=p, placed=True, edited=True, based=True)
        try:
            check_batch(batch, stats, seqs, alns, want, case=str(change))
        finally:
            batch.free()


def test_the_planted_reads_on_the_device_equal_the_definition(hip):
    """The 300 reads of the planted-read property (tests/test_align_host.py), every parameter at its default."""
    names, lengths, fasta, ref, reads, truth = ac.property_inputs()
    t = ac.Table(align.params(), names, lengths, None, fasta, ref, None, None, reads, None, None, None)
    d = OnDevice(hip, t)
    try:
        seqs = [s for _, s in reads]
        alns, want = align.align_reads(seqs, ref, t.p)
        batch, stats = d.align(seqs, placed=True, edited=True, based=True)
        try:
            check_batch(batch, stats, seqs, alns, want, case="planted")
        finally:
            batch.free()
        assert want.aligned == 300
    finally:
        d.free()


# ---- through map_main -----------------------------------------------------------------------------------------------------------
def write_dbinfo(path, names, lengths):
    rows = ["Accession\tLength\tTaxID\tLineage\tTaxID_Lineage\n", "Unmapped\t0\tUnmapped\t|||||||Unmapped\t|||||||Unmapped\n"]
    for g, (name, n) in enumerate(zip(names, lengths)):
        rows.append("\t".join([name, str(n), "%d.1" % (1000 + g), "Bacteria|P|C|O|F|G%d|G%d s%d|G%d s%d str1" % (g // 4, g // 4, g, g // 4, g),
                               "2|10|20|30|40|%d|%d|%d.1" % (500 + g // 4, 1000 + g, 1000 + g)]) + "\n")
    path.write_text("".join(rows))


SIDES = ("coverage", "depth", "identity", "variants", "variant_sites", "consensus", "ani")


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """The case table of the default (k, w) as files: db_info, the reference FASTA, a FASTQ of its reads six times over under
    distinct names, its .gz, and the definition's SAM text for the same reads."""
    t = ac.table(15, 5)
    d = tmp_path_factory.mktemp("align_sample")
    write_dbinfo(d / "db_info.txt", t.names, t.lengths)
    (d / "db.fna").write_bytes(t.fasta)
    picks = [("%s_%d extra words" % (name, rep), seq) for rep in range(6) for name, seq in t.reads if len(seq) > 0]
    fastq = b"".join(b"@%s\n%s\n+\n%s\n" % (h.encode(), s, b"I" * len(s)) for h, s in picks)
    (d / "reads.fq").write_bytes(fastq)
    (d / "reads.fq.gz").write_bytes(gzip.compress(fastq[:len(fastq) // 3]) + gzip.compress(fastq[len(fastq) // 3:]))  # two members
    alns = [t.alns[h.split(" ")[0].rsplit("_", 1)[0]] for h, _ in picks]
    sam = align.sam_lines([h.encode() for h, _ in picks], [s for _, s in picks], [b"I" * len(s) for _, s in picks], t.names, t.lengths, alns)
    (d / "definition.sam").write_bytes(b"".join(sam))
    return d, t


def run_map_main(d, t, infile, tag, tmp_path, dbinfo="db_info.txt", **extra):
    out = tmp_path / tag
    out.mkdir()
    over = dict({f: str(out / f) for f in SIDES}, db=str(d / "db.fna"), sampleID="s", align_max_occ=ac.MAX_OCC, **extra)
    over["input_type"] = "sam" if infile.endswith(".sam") else "fastq"
    mp.map_main(sc.make_args(str(d / infile), str(d / dbinfo), str(out / "profile"), over))
    return {f: (out / f).read_bytes() for f in SIDES + ("profile",)}


def test_a_db_info_whose_lengths_contradict_the_fasta(hip, sample, tmp_path):
    """The subset db_info of select_db gives every accession of a genome its first row's length.  The FASTA's own lengths then
    stand in, as the @SQ lines of the definition's SAM text do: the same bytes in every output, and no accession without bases."""
    d, t = sample
    wrong = [t.lengths[0] + 7 if name in ("len70001", "tandem", "noisy") else n for name, n in zip(t.names, t.lengths)]
    write_dbinfo(d / "db_info_wrong.txt", t.names, wrong)
    want = run_map_main(d, t, "definition.sam", "sam", tmp_path, dbinfo="db_info_wrong.txt")
    assert run_map_main(d, t, "reads.fq", "fq", tmp_path, dbinfo="db_info_wrong.txt", aligner="device") == want
    assert b"len70001" in want["coverage"] and b"tandem" in want["coverage"]


@pytest.mark.parametrize("extra", [dict(), dict(side_reads="unique"), dict(multimap_iterations=3)], ids=["all", "unique", "iterated"])
def test_map_main_on_reads_equals_map_main_on_the_definitions_sam(hip, sample, tmp_path, monkeypatch, extra):
    """A FASTQ and its .gz under --aligner device with every side output: each file byte for byte what map_main writes for the SAM
    text of align.sam_lines.  No minimap2 exists on PATH.  The .gz goes up in pieces of 20 000 bytes: records cut at every piece end."""
    d, t = sample
    empty = tmp_path / "no_aligner_here"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))
    want = run_map_main(d, t, "definition.sam", "sam", tmp_path, **extra)
    assert len(want["profile"].splitlines()) > 8 and len(want["coverage"].splitlines()) > 4  # (no comparison of empty files)
    got = run_map_main(d, t, "reads.fq", "fq", tmp_path, aligner="device", **extra)
    assert got == want
    monkeypatch.setattr(mp, "ALIGN_PIECE_BYTES", 20000)
    got = run_map_main(d, t, "reads.fq.gz", "gz", tmp_path, aligner="device", **extra)
    assert got == want


def test_a_fasta_of_reads_over_several_lines(hip, sample, tmp_path):
    d, t = sample
    picks = [(name, seq) for name, seq in t.reads if len(seq) > 0]
    (d / "reads.fa").write_bytes(b"".join(b">%s\n%s\n%s\n" % (h.encode(), s[:70], s[70:]) for h, s in picks))
    sam = align.sam_lines([h.encode() for h, _ in picks], [s for _, s in picks], None, t.names, t.lengths, [t.alns[h] for h, _ in picks])
    (d / "fa.sam").write_bytes(b"".join(sam))
    want = run_map_main(d, t, "fa.sam", "sam", tmp_path)
    over = dict({f: str(tmp_path / ("fa_" + f)) for f in SIDES}, db=str(d / "db.fna"), sampleID="s", align_max_occ=ac.MAX_OCC,
                aligner="device", input_type="fasta")
    mp.map_main(sc.make_args(str(d / "reads.fa"), str(d / "db_info.txt"), str(tmp_path / "fa_profile"), over))
    assert {f: (tmp_path / ("fa_" + f)).read_bytes() for f in SIDES + ("profile",)} == want


# ---- through metalign.main ------------------------------------------------------------------------------------------------------
def test_metalign_main_needs_no_minimap2(hip, tmp_path, monkeypatch):
    """The fixture directory of the pipeline test, PATH without any minimap2: --aligner device writes the profile map_main writes
    for the definition's SAM text over the subset database; without the flag the run fails for want of the binary."""
    import subprocess
    import sys
    import util
    from metalign_amd import build_db
    from test_pipeline_gpu import _make_data_dir
    rng = np.random.default_rng(2024)
    data, gb, go, names, accs = _make_data_dir(tmp_path, rng)
    build_db.build([str(data / "organism_files" / nm) for nm in names], str(data / "sketch_table"), [21, 31], 150)
    rb, ro, src = util.sample_reads(rng, gb, go, 1200, 150, err=0.005, present=[3, 8])
    seqs = [bytes(rb[int(ro[i]):int(ro[i + 1])]) for i in range(len(ro) - 1)]
    # Every tenth read is half from one contig of its genome and half from the other: two alignments that both pass --pct_id.  The
    # reference's read loop drops the first line of the read behind one without a passing line (a read across the contigs' boundary
    # is one), so a stream of one-line reads alone would leave the profile empty; a read of two lines ends such a run.
    for i in range(0, len(seqs), 10):
        g = int(go[src[i]])
        seqs[i] = bytes(gb[g + 100 + i:g + 175 + i]) + bytes(gb[g + 4000 + i:g + 4075 + i])
    fq = tmp_path / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)))
    empty = tmp_path / "no_aligner_here"
    empty.mkdir()
    out, tmpd = tmp_path / "abundances.tsv", tmp_path / "tmp"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the command line itself, in a process of its own (stage A's read sketches leave their table-size hints with the process)
    common = [sys.executable, os.path.join(root, "scripts", "metalign.py"), str(fq), str(data), "--temp_dir", str(tmpd), "--keep_temp_files",
              "--sketch_table", str(data / "sketch_table"), "--sampleID", "s1"]
    env = dict(os.environ, PATH=str(empty))
    r = subprocess.run(common + ["--output", str(out), "--aligner", "device"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    text = out.read_text()
    # the same from the definition: the subset database and its db_info, the reads aligned on the host, their SAM text profiled
    dbinfo = tmpd / "subset_db_info.txt"
    args = sc.make_args("x.sam", str(dbinfo), "-", {})
    acc2info, _ = mp.get_acc2info(args)
    order = list(acc2info)
    fasta = refseq.read_bytes(str(tmpd / "cmashed_db.fna"))
    # (the subset db_info gives every accession of a genome its first row's length, as the reference writes it: the lengths of the
    # FASTA's own records stand in for the @SQ lines an aligner would write)
    true = {name.decode(): len(bases) for name, bases in reversed(refseq.records_of(fasta))}
    lengths = [true.get(a, acc2info[a][0]) for a in order]
    ref = refseq.parse(fasta, {a: i for i, a in enumerate(order)}, lengths)
    alns, stats = align.align_reads(seqs, ref, align.params())
    print("definition: %s; reference records %s; subset db_info:\n%s\nprofile:\n%s" % (stats, ref.counters, dbinfo.read_text(), text))
    assert sum(ref.loaded) == len(order) - 1  # (every row but Unmapped)
    assert stats.aligned > 1100
    sam = tmp_path / "definition.sam"
    sam.write_bytes(b"".join(align.sam_lines([b"r%d" % i for i in range(len(seqs))], seqs, [b"I" * len(s) for s in seqs], order, lengths, alns)))
    out2 = tmp_path / "from_sam.tsv"
    mp.map_main(mp.profile_parseargs([str(sam), str(data), "--dbinfo", str(dbinfo), "--output", str(out2), "--sampleID", "s1"]))
    print("from the definition's SAM text:\n%s" % out2.read_text())
    assert out2.read_text() == text
    strains = [ln.split("\t") for ln in text.splitlines() if "\tstrain\t" in ln]
    assert {s[0] for s in strains} >= {"1001.2.1", "1004.1.1"}
    # the default aligner is an external program, and none is installed
    r = subprocess.run(common + ["--output", str(tmp_path / "never.tsv")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "FileNotFoundError" in r.stderr and "minimap2" in r.stderr, r.stderr[-3000:]
