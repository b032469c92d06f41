"""-m gpu: the aligner's gapped extension on the device (k_al_gap of mg_align.hip) against its definition (metalign_amd/align.py:
extend_gapped) — records, places, edits, pile entries, pool bytes and the six stats at every case of tests/align_gap_cases.py, every
band, every batch size and a few workgroups; the old entry point; the planted-indel reads; and --align_band through map_main and
metalign.main against the same runs on the definition's SAM text.  Every comparison is exact equality."""
import os

import numpy as np
import pytest

import align_cases as ac
import align_gap_cases as gc
from metalign_amd import _hip, align, refseq
from metalign_amd import map_and_profile as mp
from test_gpu_align import SIDES, OnDevice, check_batch, run_map_main, write_dbinfo

pytestmark = pytest.mark.gpu


class GapOnDevice(OnDevice):
    def align_gapped(self, seqs, gp, p=None, **want):
        bases, offs = ac.packed(seqs)
        d_b, d_o = self.hip.array(bases if bases.size else np.zeros(8, np.uint8)), self.hip.array(offs)
        try:
            return self.hip.align_reads_gapped_dev(self.index, d_b.ptr, d_o.ptr, len(seqs), p or self.t.p, gp, **want)
        finally:
            d_b.free()
            d_o.free()


@pytest.fixture(scope="module")
def dev(hip):
    d = GapOnDevice(hip, ac.table(gc.K, gc.W))
    yield d
    d.free()


ALL = dict(placed=True, edited=True, based=True)


def check_gapped(dev, seqs, gp, alns, want, want_refined, case, p=None, **sides):
    sides = sides or ALL
    batch, stats, refined = dev.align_gapped(seqs, gp, p=p, **sides)
    try:
        check_batch(batch, stats, seqs, alns, want, placed=sides.get("placed", False), edited=sides.get("edited", False),
                    based=sides.get("based", False), case=case)
        assert refined == want_refined, (case, refined, want_refined)
    finally:
        batch.free()


@pytest.mark.parametrize("grid", [0, 1, 2])
@pytest.mark.parametrize("band", gc.BANDS)
def test_every_case_at_every_batch_size(dev, knobs, band, grid):
    """The whole case table — the ungapped aligner's reads and the reads with gaps — at this band: the six stats, records, places,
    edits, pile entries and pool equal the definition's, on the launcher's grid and with every grid cut to 1 and 2 workgroups."""
    knobs("align_grid", grid)
    gt = gc.table(band)
    for n in ac.BATCH_SIZES + [len(gt.reads)]:
        names, seqs, alns, want, refined = gc.batch_of(gt, n)
        check_gapped(dev, seqs, gt.gp, alns, want, refined, "band=%d n=%d grid=%d" % (band, n, grid))
    assert refined > 200 and want.accepted > refined and want.records > want.aligned > 100


@pytest.mark.parametrize("want", [dict(), dict(placed=True), dict(edited=True), dict(based=True), dict(placed=True, edited=True),
                                  dict(placed=True, based=True), dict(edited=True, based=True), ALL],
                         ids=["none", "places", "edits", "bases", "places_edits", "places_bases", "edits_bases", "all"])
def test_every_subset_of_the_side_arrays_gives_the_same_records(dev, want):
    gt = gc.table(8)
    names, seqs, alns, stats_want, refined = gc.batch_of(gt, len(gt.reads))
    batch, stats, got_refined = dev.align_gapped(seqs, gt.gp, **want)
    try:
        check_batch(batch, stats, seqs, alns, stats_want, placed=want.get("placed", False), edited=want.get("edited", False),
                    based=want.get("based", False), case=str(want))
        assert got_refined == refined
    finally:
        batch.free()


def test_batches_appended_and_halved_give_one_batch(dev, knobs):
    """Three calls into one batch; and a candidate budget so small that the library halves every range of reads down to single
    reads, so that refined candidates lie on both sides of every cut."""
    gt = gc.table(8)
    names, seqs, alns, want, refined = gc.batch_of(gt, len(gt.reads))
    cuts = [0, 7, 90, len(seqs)]
    batch, total, total_refined = None, np.zeros(5, dtype=np.int64), 0
    for lo, hi in zip(cuts, cuts[1:]):
        batch, stats, r = dev.align_gapped(seqs[lo:hi], gt.gp, batch=batch, **ALL)
        total += np.asarray(stats)
        total_refined += r
    try:
        check_batch(batch, align.Stats(*total.tolist()), seqs, alns, want, case="appended")
        assert total_refined == refined
    finally:
        batch.free()
    t = gt.t

    def raw(seq):  # the candidates a read emits before they are made distinct
        L = len(seq)
        if L < t.p.k or L > align.MAX_READ:
            return 0
        occ = [len(t.index.get(key, ())) for key, _, _ in align.minimizers(refseq.codes_of(seq), t.p.k, t.p.w)]
        return sum(n for n in occ if n <= t.p.max_occ)

    most = max(raw(s) for s in set(seqs))
    knobs("align_batch_cands", most)
    check_gapped(dev, seqs, gt.gp, alns, want, refined, "halved")
    assert sum(1 for name in names if gt.stats_of[name][2]) > 100  # (reads with refined candidates all along the batch)


def test_a_workspace_that_does_not_fit_halves_the_range(dev, knobs):
    """The budget of the refined candidates' workspace (4 + 2 L + 2 B bytes each) set to what the hungriest single read needs: the
    library halves every range of reads whose workspace takes more, down to single reads, with refined candidates on both sides
    of every cut; the records and the six stats stay those of one call.  One byte less, and that read cannot be aligned at all."""
    gt = gc.table(8)
    names, seqs, alns, want, refined = gc.batch_of(gt, len(gt.reads))
    need = {name: gt.stats_of[name][2] * (4 + 2 * len(seq) + 2 * gt.gp.band) for name, seq in gt.reads}
    most = max(need.values())
    assert sum(need.values()) > 8 * most  # (at least three levels of halving)
    knobs("align_gap_bytes", most)
    check_gapped(dev, seqs, gt.gp, alns, want, refined, "workspace halved")
    knobs("align_gap_bytes", most - 1)
    with pytest.raises(_hip.HipError) as e:
        dev.align_gapped(seqs, gt.gp, **ALL)
    assert e.value.code == _hip.ERR_NOMEM and str(most) in str(e.value)


def test_a_batch_in_which_no_candidate_is_refined(dev):
    gt = gc.table(8)
    seqs = gc.unrefined_reads(gt.t)
    alns, want, refined = align.align_reads_gapped(seqs, gt.t.ref, gt.t.p, gt.gp, index=gt.t.index)
    assert refined == 0 and want.aligned == len(seqs) and want.accepted >= len(seqs)
    check_gapped(dev, seqs, gt.gp, alns, want, 0, "unrefined")


def test_the_old_entry_point_and_band_zero_give_identical_batches(dev):
    gt = gc.table(8)
    seqs = [s for _, s in gt.reads]
    alns, want = align.align_reads(seqs, gt.t.ref, gt.t.p, index=gt.t.index)
    old, old_stats = dev.align(seqs, **ALL)
    new, new_stats, refined = dev.align_gapped(seqs, align.gap_params(0, 0, 64), **ALL)
    try:
        check_batch(old, old_stats, seqs, alns, want, case="old")
        check_batch(new, new_stats, seqs, alns, want, case="band 0")
        assert refined == 0 and np.array_equal(old.download(), new.download()) and np.array_equal(old.places(), new.places())
        assert np.array_equal(old.edits(), new.edits()) and old.bases()[1] == new.bases()[1] and np.array_equal(old.bases()[0], new.bases()[0])
    finally:
        old.free()
        new.free()


def test_gap_values_out_of_range_are_refused(dev):
    bases, offs = ac.packed([b"ACGT" * 10])
    d_b, d_o = dev.hip.array(bases), dev.hip.array(offs)
    try:
        for bad in ((32, 6, 1), (8, 65, 1), (8, 6, 0), (8, 6, 65), (0, 6, 0), (2 ** 32 - 1, 6, 1)):
            with pytest.raises(_hip.HipError) as e:
                dev.hip.align_reads_gapped_dev(dev.index, d_b.ptr, d_o.ptr, 1, dev.t.p, align.GapParams(*bad))
            assert e.value.code == _hip.ERR_ARG
        batch, stats, refined = dev.hip.align_reads_gapped_dev(dev.index, d_b.ptr, d_o.ptr, 1, dev.t.p, align.GapParams(31, 64, 64))
        batch.free()
    finally:
        d_b.free()
        d_o.free()


@pytest.mark.parametrize("change,gap", [(dict(), (8, 0, 1)), (dict(), (8, 0, 2)), (dict(), (4, 64, 64)), (dict(mismatch=1), (8, 1, 1)),
                                        (dict(mismatch=64), (31, 6, 1)), (dict(min_score=1, max_secondary=15, sec_pct=0), (2, 3, 2))],
                         ids=["open0", "open0_ext2", "dear", "mismatch1", "mismatch64", "keep_all"])
def test_other_costs_and_parameters(dev, change, gap):
    """The reads with gaps (not the 1024-base ones) under other gap costs, mismatch costs and selection parameters."""
    gt = gc.table(8)
    t, gp = gt.t, align.gap_params(*gap)
    seqs = [s for _, s in gt.reads if len(s) <= 300]
    p = t.p._replace(**change)
    alns, want, refined = align.align_reads_gapped(seqs, t.ref, p, gp, index=t.index)
    assert refined > 100
    check_gapped(dev, seqs, gp, alns, want, refined, str((change, gap)), p=p)


def test_the_planted_indel_reads_on_the_device_equal_the_definition(hip):
    """The 300 reads of the planted-indel property (tests/test_align_gap_host.py), every parameter at its default, band 8."""
    names, lengths, fasta, ref, reads, truth = gc.property_inputs()
    t = ac.Table(align.params(), names, lengths, None, fasta, ref, None, None, reads, None, None, None)
    d = GapOnDevice(hip, t)
    try:
        seqs, gp = [s for _, s in reads], gc.gap_params_of(gc.PROPERTY_BAND)
        alns, want, refined = align.align_reads_gapped(seqs, ref, t.p, gp)
        check_gapped(d, seqs, gp, alns, want, refined, "planted")
        assert sum(gc.found(kept, a) for kept, a in zip(alns, truth)) >= 285 and refined > 300
    finally:
        d.free()


# ---- through map_main -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """The case table at band 8 as files: db_info, the reference FASTA, a FASTQ of its reads twice over under distinct names, and
    the definition's SAM text for the same reads."""
    gt = gc.table(8)
    t = gt.t
    d = tmp_path_factory.mktemp("align_gap_sample")
    write_dbinfo(d / "db_info.txt", t.names, t.lengths)
    (d / "db.fna").write_bytes(t.fasta)
    picks = [("%s_%d extra" % (name, rep), name, seq) for rep in range(2) for name, seq in gt.reads if len(seq) > 0]
    (d / "reads.fq").write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (h.encode(), s, b"I" * len(s)) for h, _, s in picks))
    sam = align.sam_lines([h.encode() for h, _, _ in picks], [s for _, _, s in picks], [b"I" * len(s) for _, _, s in picks], t.names,
                          t.lengths, [gt.alns[name] for _, name, _ in picks])
    cigars = [ln.split(b"\t")[5] for ln in sam if not ln.startswith(b"@")]
    assert sum(1 for c in cigars if b"D" in c or b"I" in c) > 100
    (d / "definition.sam").write_bytes(b"".join(sam))
    return d, t


@pytest.mark.parametrize("extra", [dict(), dict(side_reads="unique")], ids=["all", "unique"])
def test_map_main_with_the_band_equals_map_main_on_the_definitions_sam(hip, sample, tmp_path, monkeypatch, extra):
    """--aligner device --align_band 8 on a FASTQ with every side output — the profile, --coverage, --depth, --identity, --variants,
    --variant_sites, --consensus and --ani: each file byte for byte what map_main writes for the SAM text of align.sam_lines."""
    d, t = sample
    empty = tmp_path / "no_aligner_here"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))
    want = run_map_main(d, t, "definition.sam", "sam", tmp_path, **extra)
    assert len(want["profile"].splitlines()) > 8 and len(want["coverage"].splitlines()) > 4 and len(want["variants"].splitlines()) > 4
    got = run_map_main(d, t, "reads.fq", "fq", tmp_path, aligner="device", align_band=8, **extra)
    assert got == want
    assert set(SIDES) >= {"coverage", "identity", "variants", "consensus"}
    # without the band the same reads give other files: the flag is what is tested
    assert run_map_main(d, t, "reads.fq", "fq0", tmp_path, aligner="device", **extra) != want


# ---- through metalign.main ------------------------------------------------------------------------------------------------------
def test_metalign_main_with_the_band(hip, tmp_path):
    """The fixture directory of the pipeline test, every fifth read with a deletion or an insertion of 1 .. 8 bases:
    --aligner device --align_band 8 writes the profile map_main writes for the definition's SAM text over the subset database."""
    import subprocess
    import sys
    import util
    import stage_c_checks as sc
    from metalign_amd import build_db
    from test_pipeline_gpu import _make_data_dir
    rng = np.random.default_rng(77)
    data, gb, go, names, accs = _make_data_dir(tmp_path, rng)
    build_db.build([str(data / "organism_files" / nm) for nm in names], str(data / "sketch_table"), [21, 31], 150)
    rb, ro, src = util.sample_reads(rng, gb, go, 600, 150, err=0.005, present=[3, 8])
    seqs = [bytes(rb[int(ro[i]):int(ro[i + 1])]) for i in range(len(ro) - 1)]
    for i in range(0, len(seqs), 5):
        size, s = 1 + (i // 5) % 8, seqs[i]
        seqs[i] = s[:70] + s[70 + size:] if (i // 5) % 2 else s[:70] + b"ACGTACGT"[:size] + s[70:150 - size]
    # (a read of two lines ends the run of one-line reads the reference's loop would drop, as in the ungapped test)
    for i in range(3, len(seqs), 10):
        g = int(go[src[i]])
        seqs[i] = bytes(gb[g + 100 + i:g + 175 + i]) + bytes(gb[g + 4000 + i:g + 4075 + i])
    fq = tmp_path / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs)))
    out, tmpd = tmp_path / "abundances.tsv", tmp_path / "tmp"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts", "metalign.py"), str(fq), str(data), "--temp_dir", str(tmpd), "--keep_temp_files",
           "--sketch_table", str(data / "sketch_table"), "--sampleID", "s1", "--output", str(out), "--aligner", "device", "--align_band", "8"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    dbinfo = tmpd / "subset_db_info.txt"
    acc2info, _ = mp.get_acc2info(sc.make_args("x.sam", str(dbinfo), "-", {}))
    order = list(acc2info)
    fasta = refseq.read_bytes(str(tmpd / "cmashed_db.fna"))
    true = {name.decode(): len(bases) for name, bases in reversed(refseq.records_of(fasta))}
    lengths = [true.get(a, acc2info[a][0]) for a in order]
    ref = refseq.parse(fasta, {a: i for i, a in enumerate(order)}, lengths)
    alns, stats, refined = align.align_reads_gapped(seqs, ref, align.params(), align.gap_params(8))
    print("definition: %s, %d refined" % (stats, refined))
    assert stats.aligned > 550 and refined > 100
    assert sum(1 for kept in alns[::5] if kept and isinstance(kept[0], align.GapAln) and kept[0].e - kept[0].b >= 140) > 100
    sam = tmp_path / "definition.sam"
    sam.write_bytes(b"".join(align.sam_lines([b"r%d" % i for i in range(len(seqs))], seqs, [b"I" * len(s) for s in seqs], order, lengths, alns)))
    out2 = tmp_path / "from_sam.tsv"
    mp.map_main(mp.profile_parseargs([str(sam), str(data), "--dbinfo", str(dbinfo), "--output", str(out2), "--sampleID", "s1"]))
    assert out2.read_text() == out.read_text() and "\tstrain\t" in out.read_text()
