"""-m gpu: the aligner's paired-end mode on the device (k_al_rescue_mark, k_al_rescue and k_al_select_pair of mg_align.hip) against its
definition (metalign_amd/align.py: rescue_pair, select_pair) — the eight stats, records, places, edits, pile entries and pool at
every case of tests/align_pair_cases.py under every parameter set, a few workgroups, every subset of the side arrays, batches
appended and halved at even cuts; the refusals; the old entry points; the rescue property; and --align_pairs interleaved through
map_main and metalign.main against the same runs on the definition's pair SAM text.  Every comparison is exact equality."""
import os

import numpy as np
import pytest

import align_cases as ac
import align_pair_cases as pc
import stage_c_checks as sc
from metalign_amd import _hip, align, refseq
from metalign_amd import map_and_profile as mp
from test_gpu_align import SIDES, OnDevice, write_dbinfo

pytestmark = pytest.mark.gpu
ALL = dict(placed=True, edited=True, based=True)


class PairOnDevice(OnDevice):
    def align_paired(self, seqs, gp, pp, p=None, **want):
        bases, offs = ac.packed(seqs)
        d_b, d_o = self.hip.array(bases if bases.size else np.zeros(8, np.uint8)), self.hip.array(offs)
        try:
            return self.hip.align_reads_paired_dev(self.index, d_b.ptr, d_o.ptr, len(seqs), p or self.t.p, gp, pp, **want)
        finally:
            d_b.free()
            d_o.free()


@pytest.fixture(scope="module")
def dev(hip):
    d = PairOnDevice(hip, pc.table())
    yield d
    d.free()


def check_pair_batch(batch, stats, pstats, seqs, alns, proper, want, pwant, placed=True, edited=True, based=True, case=""):
    recs, places, edits, entries, pool = align.records(seqs, alns, proper)
    assert (stats, pstats) == (want, pwant), (case, stats, pstats, want, pwant)
    assert batch.count == len(recs) and np.array_equal(batch.download(), recs), case
    if placed:
        assert np.array_equal(batch.places(), places), case
    if edited:
        assert np.array_equal(batch.edits(), edits), case
    if based:
        got_entries, got_pool = batch.bases()
        assert np.array_equal(got_entries, entries) and got_pool == pool, case


def check_paired(dev, ans, names, case, **sides):
    sides = sides or ALL
    seqs, alns, proper, want, pwant = pc.batch_of(ans, names)
    batch, stats, pstats = dev.align_paired(seqs, ans.gp, ans.pp, **sides)
    try:
        check_pair_batch(batch, stats, pstats, seqs, alns, proper, want, pwant, placed=sides.get("placed", False),
                         edited=sides.get("edited", False), based=sides.get("based", False), case=case)
    finally:
        batch.free()
    return want, pwant


@pytest.mark.parametrize("grid", [0, 1, 2])
@pytest.mark.parametrize("params", pc.PARAM_SETS, ids=lambda x: "I%d_R%d_B%d" % x)
def test_every_case_under_every_parameter_set(dev, knobs, params, grid):
    """The whole pair table — mates of 15 to 1024 bases, windows of 1, 63, 64, 65 and (I = 8192) more than 7000 diagonals, both
    orientations, the accessions' ends, the tandem repeat, the twins — in one batch, in batches of 1, 32 and 33 pairs, on the
    launcher's grids and with every grid cut to 1 and 2 workgroups."""
    knobs("align_grid", grid)
    ans, names = pc.answers(*params), pc.all_names()
    want, pwant = check_paired(dev, ans, names, "%s grid=%d" % (params, grid))
    assert want.records > 150 and (pwant.rescued > 15 or params[1] == 0) and pwant.proper > 15
    for n in (0, 1, 32, 33):
        check_paired(dev, ans, [names[(7 * i) % len(names)] for i in range(n)], "%s grid=%d n=%d" % (params, grid, n))


@pytest.mark.parametrize("want", [dict(), dict(placed=True), dict(edited=True), dict(based=True), dict(placed=True, edited=True),
                                  dict(placed=True, based=True), dict(edited=True, based=True), ALL],
                         ids=["none", "places", "edits", "bases", "places_edits", "places_bases", "edits_bases", "all"])
def test_every_subset_of_the_side_arrays_gives_the_same_records(dev, want):
    seqs, alns, proper, stats_want, pwant = pc.batch_of(pc.answers(1000, 2, 8), pc.all_names())
    batch, stats, pstats = dev.align_paired(seqs, align.gap_params(8), align.pair_params(1, 1000, 2), **want)
    try:
        check_pair_batch(batch, stats, pstats, seqs, alns, proper, stats_want, pwant, placed=want.get("placed", False),
                         edited=want.get("edited", False), based=want.get("based", False), case=str(want))
    finally:
        batch.free()


def raw_candidates(t, seq):
    """The candidates a read emits before they are made distinct."""
    if len(seq) < t.p.k or len(seq) > align.MAX_READ:
        return 0
    occ = [len(t.index.get(key, ())) for key, _, _ in align.minimizers(refseq.codes_of(seq), t.p.k, t.p.w)]
    return sum(n for n in occ if n <= t.p.max_occ)


def test_batches_appended_and_halved_at_even_cuts(dev, knobs):
    """Three calls into one batch; then budgets so small that the library halves every range down to single pairs: of candidates,
    of the rescue tasks' bytes (72 each), and of the refined candidates' workspace.  One byte less than the hungriest pair needs,
    and that pair cannot be aligned at all."""
    ans, names, t = pc.answers(1000, 2, 8), pc.all_names(), pc.table()
    seqs, alns, proper, want, pwant = pc.batch_of(ans, names)
    cuts = [0, 14, 180, len(seqs)]
    batch, total, ptotal = None, np.zeros(5, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for lo, hi in zip(cuts, cuts[1:]):
        batch, stats, pstats = dev.align_paired(seqs[lo:hi], ans.gp, ans.pp, batch=batch, **ALL)
        total += np.asarray(stats)
        ptotal += np.asarray(pstats)
    try:
        check_pair_batch(batch, align.Stats(*total.tolist()), align.PairStats(*ptotal.tolist()), seqs, alns, proper, want, pwant, case="appended")
    finally:
        batch.free()
    most = max(raw_candidates(t, m1) + raw_candidates(t, m2) for _, m1, m2 in t.pairs)
    knobs("align_batch_cands", most)
    check_paired(dev, ans, names, "candidates halved")
    knobs("align_batch_cands", most - 1)
    with pytest.raises(_hip.HipError) as e:
        dev.align_paired(seqs, ans.gp, ans.pp, **ALL)
    assert e.value.code == _hip.ERR_NOMEM and "one pair" in str(e.value)
    knobs("align_batch_cands", 0)
    tasks = max(ans.counts[n][4] for n in names)
    assert tasks >= 2 and sum(ans.counts[n][4] for n in names) > 8 * tasks  # (at least three levels of halving)
    knobs("align_rescue_bytes", 72 * tasks)
    check_paired(dev, ans, names, "tasks halved")
    knobs("align_rescue_bytes", 72 * tasks - 1)
    with pytest.raises(_hip.HipError) as e:
        dev.align_paired(seqs, ans.gp, ans.pp, **ALL)
    assert e.value.code == _hip.ERR_NOMEM and str(72 * tasks) in str(e.value) and "one pair" in str(e.value)
    knobs("align_rescue_bytes", 0)
    knobs("align_gap_bytes", 4 * (4 + 2 * 1024 + 2 * 8))  # more than any pair's refined candidates take (3888 at the most), less than half of what the batch's do
    check_paired(dev, ans, names, "workspace halved")


def test_odd_read_counts_and_values_out_of_range_are_refused(dev):
    bases, offs = ac.packed([b"ACGT" * 10] * 3)
    d_b, d_o = dev.hip.array(bases), dev.hip.array(offs)
    gp = align.gap_params(8)
    try:
        for n, bad in ((3, (1, 1000, 2)), (1, (1, 1000, 2)), (2, (1, 0, 2)), (2, (1, 8193, 2)), (2, (1, 1000, 9)), (2, (2, 1000, 2)),
                       (2, (1, 2 ** 32 - 1, 2))):
            with pytest.raises(_hip.HipError) as e:
                dev.hip.align_reads_paired_dev(dev.index, d_b.ptr, d_o.ptr, n, dev.t.p, gp, align.PairParams(*bad))
            assert e.value.code == _hip.ERR_ARG, bad
        for n, good in ((2, (1, 1, 0)), (2, (1, 8192, 8)), (0, (1, 1000, 2)), (3, (0, 1000, 2))):
            batch, stats, pstats = dev.hip.align_reads_paired_dev(dev.index, d_b.ptr, d_o.ptr, n, dev.t.p, gp, align.PairParams(*good))
            assert stats.reads == n
            batch.free()
    finally:
        d_b.free()
        d_o.free()


def test_without_pairs_the_new_entry_point_is_the_gapped_call(dev):
    """pairs == NULL, and interleaved == 0 whatever the other fields hold (out of range among them), on an odd number of reads:
    the batch of mg_align_reads_gapped_dev, array by array, and no rescued candidate or proper pair."""
    ans = pc.answers(1000, 2, 8)
    seqs = pc.batch_of(ans, pc.all_names())[0][:-1]
    bases, offs = ac.packed(seqs)
    d_b, d_o = dev.hip.array(bases), dev.hip.array(offs)
    alns, want, refined = align.align_reads_gapped(seqs, dev.t.ref, dev.t.p, ans.gp, index=dev.t.index)
    try:
        old, old_stats, old_refined = dev.hip.align_reads_gapped_dev(dev.index, d_b.ptr, d_o.ptr, len(seqs), dev.t.p, ans.gp, **ALL)
        assert (old_stats, old_refined) == (want, refined) and np.array_equal(old.download(), align.records(seqs, alns)[0])
        for pairs in (None, align.PairParams(0, 1000, 2), align.PairParams(0, 0, 99), align.PairParams(0, 2 ** 32 - 1, 2 ** 32 - 1)):
            new, stats, pstats = dev.hip.align_reads_paired_dev(dev.index, d_b.ptr, d_o.ptr, len(seqs), dev.t.p, ans.gp, pairs, **ALL)
            try:
                assert (stats, pstats) == (want, (refined, 0, 0)), pairs
                assert np.array_equal(old.download(), new.download()) and np.array_equal(old.places(), new.places())
                assert np.array_equal(old.edits(), new.edits()) and old.bases()[1] == new.bases()[1]
                assert np.array_equal(old.bases()[0], new.bases()[0])
            finally:
                new.free()
        old.free()
    finally:
        d_b.free()
        d_o.free()


@pytest.mark.parametrize("change", [dict(sec_pct=0, max_secondary=15), dict(max_secondary=0), dict(sec_pct=100, max_secondary=1),
                                    dict(mismatch=1, min_score=60)], ids=["keep_all", "primaries", "equal_only", "mismatch1"])
def test_other_selection_parameters(dev, change):
    t = pc.table()
    p, gp, pp = t.p._replace(**change), align.gap_params(8), align.pair_params(1, 1000, 2)
    seqs = [s for _, m1, m2 in t.pairs for s in (m1, m2) if max(len(m1), len(m2)) <= 150]
    alns, proper, want, pwant = align.align_reads_paired(seqs, t.ref, p, gp, pp, index=t.index)
    batch, stats, pstats = dev.align_paired(seqs, gp, pp, p=p, **ALL)
    try:
        check_pair_batch(batch, stats, pstats, seqs, alns, proper, want, pwant, case=str(change))
    finally:
        batch.free()
    assert pwant.proper > 20 and pwant.rescued > 10


def test_the_rescue_property_on_the_device_equals_the_definition(hip):
    """The 300 pairs of the rescue property (tests/test_align_pair_host.py), every parameter at its default: R = 2 and R = 0."""
    names, lengths, fasta, ref, seqs, truth = pc.property_inputs()
    t = ac.Table(align.params(), names, lengths, None, fasta, ref, None, None, None, None, None, None)
    d = PairOnDevice(hip, t)
    try:
        index = align.build_index(ref, t.p.k, t.p.w)
        for R, least in ((2, 295), (0, 0)):
            gp, pp = align.gap_params(), align.pair_params(1, 1000, R)
            alns, proper, want, pwant = align.align_reads_paired(seqs, ref, t.p, gp, pp, index=index)
            batch, stats, pstats = d.align_paired(seqs, gp, pp, **ALL)
            try:
                check_pair_batch(batch, stats, pstats, seqs, alns, proper, want, pwant, case="property R=%d" % R)
            finally:
                batch.free()
            found = sum(pc.planted(alns[2 * i], alns[2 * i + 1], proper[i], truth[i]) for i in range(300))
            assert found >= least and pstats.proper == found and (R or found == 0)
    finally:
        d.free()


# ---- through map_main -----------------------------------------------------------------------------------------------------------
PARAMS = (1000, 2, 8)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """The pair table as files: db_info, the reference FASTA, an interleaved FASTQ of its pairs twice over under distinct names, the
    same as a FASTA of several lines, and the definition's pair SAM text for them."""
    t, ans = pc.table(), pc.answers(*PARAMS)
    d = tmp_path_factory.mktemp("align_pair_sample")
    write_dbinfo(d / "db_info.txt", t.names, t.lengths)
    (d / "db.fna").write_bytes(t.fasta)
    picks = [("%s_%d" % (name, rep), name, m1, m2) for rep in range(2) for name, m1, m2 in t.pairs if m1 and m2]
    headers = [b"%s/%d extra" % (h.encode(), m + 1) for h, _, _, _ in picks for m in (0, 1)]
    seqs = [s for _, _, m1, m2 in picks for s in (m1, m2)]
    (d / "reads.fq").write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (h, s, b"I" * len(s)) for h, s in zip(headers, seqs)))
    (d / "reads.fa").write_bytes(b"".join(b">%s\n%s\n%s\n" % (h, s[:70], s[70:]) for h, s in zip(headers, seqs)))
    alns = [k for _, name, _, _ in picks for k in ans.kept[name]]
    proper = [ans.proper[name] for _, name, _, _ in picks]
    for tag, quals in (("fq", [b"I" * len(s) for s in seqs]), ("fa", None)):
        sam = align.sam_lines(headers, seqs, quals, t.names, t.lengths, alns, proper)
        (d / ("definition_%s.sam" % tag)).write_bytes(b"".join(sam))
    flags = [int(ln.split(b"\t")[1]) for ln in sam if not ln.startswith(b"@")]
    assert sum(1 for f in flags if f & 2) > 300 and sum(1 for f in flags if f & 8) > 10 and all(f & 1 for f in flags)
    (d / "odd.fq").write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (h, s, b"I" * len(s)) for h, s in list(zip(headers, seqs))[:7]))
    return d, t


def run(d, infile, tag, tmp_path, **extra):
    out = tmp_path / tag
    out.mkdir()
    over = dict({f: str(out / f) for f in SIDES}, db=str(d / "db.fna"), sampleID="s", **extra)
    over["input_type"] = "sam" if infile.endswith(".sam") else "fasta" if infile.endswith(".fa") else "fastq"
    mp.map_main(sc.make_args(str(d / infile), str(d / "db_info.txt"), str(out / "profile"), over))
    return {f: (out / f).read_bytes() for f in SIDES + ("profile",)}


PAIR_FLAGS = dict(aligner="device", align_band=8, align_pairs="interleaved", align_max_insert=1000, align_rescue=2)


@pytest.mark.parametrize("piece", [None, 7001, 2500], ids=["whole", "pieces7001", "pieces2500"])
def test_map_main_with_pairs_equals_map_main_on_the_definitions_pair_sam(hip, sample, tmp_path, monkeypatch, piece):
    """--aligner device --align_pairs interleaved on an interleaved FASTQ with every side output: each file byte for byte what
    map_main writes for the SAM text of align.sam_lines in pair mode.  In pieces of 7001 and 2500 bytes the text is cut inside
    records and between the mates of a pair: pieces that parse to an odd number of reads carry their last read on."""
    d, t = sample
    want = run(d, "definition_fq.sam", "sam", tmp_path)
    assert len(want["profile"].splitlines()) > 8 and len(want["coverage"].splitlines()) > 4 and len(want["variants"].splitlines()) > 4
    if piece:
        monkeypatch.setattr(mp, "ALIGN_PIECE_BYTES", piece)
        odd = []
        real = _hip.Hip.parse_reads_prefix_dev

        def spy(self, *a):
            reads, used = real(self, *a)
            odd.append(reads.count % 2)
            return reads, used
        monkeypatch.setattr(_hip.Hip, "parse_reads_prefix_dev", spy)
    assert run(d, "reads.fq", "fq", tmp_path, **PAIR_FLAGS) == want
    if piece:
        assert sum(odd[:-1]) > 5 and len(odd) > 20  # (cuts that left an odd read)
    else:  # without the flag the same reads give other files: the flag is what is tested
        assert run(d, "reads.fq", "fq0", tmp_path, **dict(PAIR_FLAGS, align_pairs="none")) != want


def test_map_main_with_pairs_on_a_fasta_of_several_lines(hip, sample, tmp_path, monkeypatch):
    d, t = sample
    want = run(d, "definition_fa.sam", "sam", tmp_path)
    monkeypatch.setattr(mp, "ALIGN_PIECE_BYTES", 3001)
    assert run(d, "reads.fa", "fa", tmp_path, **PAIR_FLAGS) == want


def test_an_odd_number_of_reads_in_the_file_is_an_error_that_names_it(hip, sample, tmp_path):
    d, t = sample
    with pytest.raises(SystemExit) as e:
        run(d, "odd.fq", "odd", tmp_path, **PAIR_FLAGS)
    assert "odd.fq" in str(e.value) and "odd number" in str(e.value)


# ---- through metalign.main ------------------------------------------------------------------------------------------------------
def test_metalign_main_with_pairs(hip, tmp_path):
    """The fixture directory of the pipeline test, 300 interleaved pairs of its genomes 3 and 8, every third mate 2 without a seed:
    --aligner device --align_pairs interleaved --align_band 8 writes the profile map_main writes for the definition's pair SAM text
    over the subset database."""
    import subprocess
    import sys
    from metalign_amd import build_db
    from test_pipeline_gpu import _make_data_dir
    rng = np.random.default_rng(404)
    data, gb, go, names, accs = _make_data_dir(tmp_path, rng)
    build_db.build([str(data / "organism_files" / nm) for nm in names], str(data / "sketch_table"), [21, 31], 150)
    seqs = []
    for i in range(300):
        g = int(go[(3, 8)[i % 2]])
        genome = bytes(gb[g:g + 3000])  # (the first of its two contigs)
        F, at = int(rng.integers(300, 600)), int(rng.integers(50, 2350))
        m1, m2 = pc.mates(genome, at, F, 150, 150, flip=i % 4 >= 2)
        seqs += [m1, pc.unseedable(m2) if i % 3 == 0 else m2]
    fq = tmp_path / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i // 2, i % 2 + 1, s, b"I" * len(s)) for i, s in enumerate(seqs)))
    out, tmpd = tmp_path / "abundances.tsv", tmp_path / "tmp"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts", "metalign.py"), str(fq), str(data), "--temp_dir", str(tmpd), "--keep_temp_files",
           "--sketch_table", str(data / "sketch_table"), "--sampleID", "s1", "--output", str(out), "--aligner", "device", "--align_band", "8",
           "--align_pairs", "interleaved"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    dbinfo = tmpd / "subset_db_info.txt"
    acc2info, _ = mp.get_acc2info(sc.make_args("x.sam", str(dbinfo), "-", {}))
    order = list(acc2info)
    fasta = refseq.read_bytes(str(tmpd / "cmashed_db.fna"))
    true = {name.decode(): len(bases) for name, bases in reversed(refseq.records_of(fasta))}
    lengths = [true.get(a, acc2info[a][0]) for a in order]
    ref = refseq.parse(fasta, {a: i for i, a in enumerate(order)}, lengths)
    alns, proper, stats, pstats = align.align_reads_paired(seqs, ref, align.params(), align.gap_params(8), align.pair_params(1))
    print("definition: %s, %s" % (stats, pstats))
    assert pstats.proper > 250 and pstats.rescued > 80
    sam = tmp_path / "definition.sam"
    sam.write_bytes(b"".join(align.sam_lines([b"r%d/%d" % (i // 2, i % 2 + 1) for i in range(len(seqs))], seqs, [b"I" * len(s) for s in seqs],
                                             order, lengths, alns, proper)))
    out2 = tmp_path / "from_sam.tsv"
    mp.map_main(mp.profile_parseargs([str(sam), str(data), "--dbinfo", str(dbinfo), "--output", str(out2), "--sampleID", "s1"]))
    assert out2.read_text() == out.read_text() and "\tstrain\t" in out.read_text()
