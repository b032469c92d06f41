"""-m gpu: BAM READS files for stages A / B, unpacked on the device (metalign_amd/csrc/mg_bam.hip: k_bam_seq_len / k_bam_seq_unpack).

A BAM reads file means what `samtools fastq` (-F 0x900) writes for it.  The reads are built first (tests/bamreads.py) and written
twice, as FASTQ text and as a BAM holding them the way aligners store them (reverse strand stored reverse-complemented,
secondary / supplementary records with other SEQ, SEQ '*').  Every expectation is the original FASTQ through the existing path,
and the oracle where one exists; metalign_amd/bam.py is not used as the oracle."""
import os
import stat
import subprocess
import sys

import numpy as np
import pytest

import bamgen
import bamreads
import util
from metalign_amd import _hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEFAULT_INFLATE = dict(chunk_bytes=32 << 10, stage_bytes=-1, ratio=10, on=1, lane_jobs=1 << 40)


@pytest.fixture(scope="module")
def case():
    reads, gb, go = bamreads.make_reads(seed=11, ntiles=60, nlong=4)
    return reads, gb, go


@pytest.fixture()
def inflate(hip):
    yield hip.inflate_config
    hip.inflate_config(**_DEFAULT_INFLATE)


def _fastq_reads(hip, reads):
    r = hip.parse_reads(bamreads.fastq_text(reads), "fastq")
    try:
        return r.download()
    finally:
        r.free()


def test_parse_bam_prefix_whole_and_in_pieces(hip, case):
    reads = case[0]
    want_b, want_o = _fastq_reads(hip, reads)
    assert np.array_equal(want_o, bamreads.bases_offsets(reads)[1])
    _, stream, n_ref = bamreads.bam_bytes(reads, seed=12, bgzf=False)
    arr = np.frombuffer(stream, dtype=np.uint8)
    d = hip.array(arr)
    try:
        whole, used = hip.parse_bam_reads_dev(d.ptr, arr.size, n_ref, final=True)
        assert used == arr.size
        b, o = whole.download()
        whole.free()
        assert np.array_equal(o, want_o) and np.array_equal(b, want_b)
        # pieces cut at arbitrary bytes: the complete records of each, the rest carried (a long read spans many pieces)
        rng = np.random.default_rng(13)
        pos, end, got = 0, 0, []
        while True:
            end = min(max(end, pos) + int(rng.integers(300, 30000)), arr.size)
            final = end == arr.size
            r, used = hip.parse_bam_reads_dev(d.ptr + pos, end - pos, n_ref, final=final)
            got.append(r.download())
            r.free()
            pos += used
            if final:
                break
        assert len(got) > 40
        cat_b = np.concatenate([g[0] for g in got])
        cat_o, at = [np.zeros(1, np.uint64)], 0
        for gb_, go_ in got:
            cat_o.append(go_[1:] + np.uint64(at))
            at += len(gb_)
        assert np.array_equal(cat_b, want_b) and np.array_equal(np.concatenate(cat_o), want_o)
        # a corrupt block_size: an error at that byte, no reads
        offs, q = [], 0
        while q < len(stream):
            offs.append(q)
            q += 4 + int.from_bytes(stream[q:q + 4], "little")
        victim = offs[len(offs) // 2]
        bad = arr.copy()
        bad[victim:victim + 4] = np.frombuffer((7).to_bytes(4, "little"), np.uint8)
        db = hip.array(bad)
        try:
            with pytest.raises(_hip.HipError) as e:
                hip.parse_bam_reads_dev(db.ptr, bad.size, n_ref, final=True)
            assert e.value.code == _hip.ERR_ARG and e.value.err_at == victim
        finally:
            db.free()
    finally:
        d.free()


def _table(hip, oracle_lib, gb, go, ks=(21, 31, 51), n=300):
    h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, ks[-1], n)
    table = hip.refdb_build(h, khi, klo, o, list(ks))
    want = oracle_lib.refpipe_build(h, khi, klo, o, list(ks))
    table.index_kmers()
    return table, want


@pytest.mark.parametrize("how", ["device inflater", "host inflater", "uncompressed", "device inflater, small pieces",
                                 "host inflater, small pieces"])
def test_counts_and_sketches_from_a_bam_equal_the_fastq_and_the_oracle(hip, oracle_lib, tmp_path, inflate, case, how):
    reads, gb, go = case
    rb, ro = bamreads.bases_offsets(reads)
    small = "small" in how
    inflate(on=0 if how.startswith("host") else 1)
    if small:
        inflate(chunk_bytes=8 << 10, stage_bytes=256 << 10)
    chunk = (1 << 16) if small else 0
    fq = tmp_path / "x.fq"
    fq.write_bytes(bamreads.fastq_text(reads))
    bm = tmp_path / "x.bam"
    bm.write_bytes(bamreads.bam_bytes(reads, seed=14, bgzf=how != "uncompressed", block=5000 if small else 65280)[0])
    # stage A by k-mer identity: the counters
    table, want_table = _table(hip, oracle_lib, gb, go)
    want, seen = oracle_lib.refpipe_count_kmers(rb, ro, 51, want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    got = []
    for path, fmt in ((fq, "fastq"), (bm, "bam")):
        kc = table.kmer_counts()
        st = hip.count_stream(kc)
        st.add_file(str(path), fmt, chunk_bytes=chunk)
        st.free()
        got.append((kc.download(), kc.stats()["kmers"]))
        kc.free()
    table.free()
    assert np.array_equal(got[1][0], got[0][0]) and got[1][1] == got[0][1]
    assert np.array_equal(got[1][0], want) and got[1][1] == seen and want.sum() > 0
    # read sketches by hash
    k = 31
    gh, _ = hip.sketch_genomes(gb, go, k, 400)
    hmax = int(gh.max())
    oh, oc, _, _ = oracle_lib.sketch_reads(rb, ro, k, hmax=hmax)
    sk = []
    for path, fmt in ((fq, "fastq"), (bm, "bam")):
        st = hip.sketch_stream([k], [hmax], 0, None, int(ro[-1]))
        st.add_file(str(path), fmt, chunk_bytes=chunk)
        (s,) = st.finish()
        s.resolve()
        sk.append(s.download())
        s.free()
        st.free()
    for h, c in sk:
        assert np.array_equal(h, oh) and np.array_equal(c, oc)
    # the whole file in one batch (the multi-rank path)
    r = hip.reads_from_bam_file(str(bm), chunk_bytes=chunk)
    b, o = r.download()
    r.free()
    assert np.array_equal(b, rb) and np.array_equal(o, ro)


def test_corrupt_and_truncated_bams_name_the_file(hip, tmp_path, case):
    reads = case[0][:500]
    data = bamgen.encode(bamreads.sam_lines(reads, seed=15))
    whole, hdr = data[0], data[1]
    cut = tmp_path / "cut.bam"
    cut.write_bytes(bamgen.bgzf(whole[:len(whole) - 37]))
    offs, q = [], hdr
    while q < len(whole):
        offs.append(q)
        q += 4 + int.from_bytes(whole[q:q + 4], "little")
    bad = bytearray(whole)
    bad[offs[len(offs) // 2]:offs[len(offs) // 2] + 4] = (7).to_bytes(4, "little")  # a block_size too small for any record
    broken = tmp_path / "broken.bam"
    broken.write_bytes(bamgen.bgzf(bytes(bad)))
    for p in (cut, broken):
        st = hip.sketch_stream([21], [_hip.U64_MAX], 0, None, 1 << 20)
        try:
            with pytest.raises(_hip.HipError, match=p.name) as e:
                st.add_file(str(p), "bam")
            assert e.value.code == _hip.ERR_ARG and "byte" in str(e.value)
        finally:
            st.free()
        with pytest.raises(_hip.HipError, match=p.name):
            hip.reads_from_bam_file(str(p))


def _select_csv(select_db, reads_path, data, tdir, tmpd, extra=()):
    args = select_db.select_parseargs([str(reads_path), str(data), "--temp_dir", str(tmpd), "--keep_temp_files",
                                       "--sketch_table", tdir] + list(extra))
    select_db.select_main(args)
    return (tmpd / "cmash_query_results.csv").read_bytes()


def test_select_main_and_metalign_on_a_bam(hip, tmp_path, monkeypatch):
    """select_main writes the CSV its FASTQ gives, on the identity table, by hash and on a plain table, streamed and piece-wise;
    metalign.main hands the aligner the reads and writes the same CAMI profile; two ranks on one GPU write world 1's CSV."""
    from metalign_amd import build_db, metalign, select_db
    from test_pipeline_gpu import _make_data_dir
    rng = np.random.default_rng(16)
    data, gb, go, names, accs = _make_data_dir(tmp_path, rng)
    rb, ro, src = util.sample_reads(rng, gb, go, 3000, 150, err=0.005, present=[3, 8])
    reads = [bytes(rb[int(ro[i]):int(ro[i + 1])]).decode() for i in range(len(ro) - 1)]
    fq = tmp_path / "sample.fq"
    fq.write_bytes(bamreads.fastq_text(reads))
    bm = tmp_path / "sample.bam"
    bm.write_bytes(bamreads.bam_bytes(reads, seed=17)[0])
    ref = str(data / "sketch_table_ref")
    plain = str(data / "sketch_table")
    build_db.main([str(data / "organism_files"), ref, "-n", "150", "-k", "21,31,51", "--reference_pipeline"])
    build_db.main([str(data / "organism_files"), plain, "-n", "150", "-k", "21,31"])
    for tdir, extra in ((ref, []), (ref, ["--kmer_match", "hash"]), (plain, [])):
        want = _select_csv(select_db, fq, data, tdir, tmp_path / "t_fq", extra)
        assert want.count(b"\n") > 2
        assert _select_csv(select_db, bm, data, tdir, tmp_path / "t_bam", extra) == want, (tdir, extra)
        if tdir == ref and not extra:
            monkeypatch.setenv("MG_NO_STREAM", "1")
            assert _select_csv(select_db, bm, data, tdir, tmp_path / "t_nostream", extra) == want
            monkeypatch.delenv("MG_NO_STREAM")
            csv_ref = want
    # metalign.main: the stub aligner keeps what it was handed and replays one SAM
    sam = tmp_path / "canned.sam"
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.6\n")
        for i, s in enumerate(reads):
            fh.write("\t".join(["r%d" % i, "0", accs[src[i]], "1", "60", "150M", "*", "0", "0", s, "I" * 150, "NM:i:0"]) + "\n")
    stub = tmp_path / "bin"
    stub.mkdir()
    handed = tmp_path / "handed"
    handed.mkdir()
    exe = stub / "minimap2"
    exe.write_text('#!/bin/sh\nfor last; do :; done\ncp "$last" %s/$(basename "$last")\ncat %s\n' % (handed, sam))
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(stub) + os.pathsep + os.environ["PATH"])
    outs = []
    for path in (fq, bm):
        out = tmp_path / ("abund_%s.tsv" % path.suffix[1:])
        metalign.main([str(path), str(data), "--output", str(out), "--temp_dir", str(tmp_path / ("m_" + path.suffix[1:])),
                       "--sketch_table", plain, "--sampleID", "s1"])
        outs.append(out.read_bytes())
    assert outs[1] == outs[0] and outs[0].startswith(b"@SampleID:s1\n")
    lines = (handed / "reads_from_bam.fq").read_bytes().split(b"\n")
    assert [ln.decode() for ln in lines[1::4]] == reads
    # two ranks on one GPU over gloo: rank 0 decodes the BAM and scatters the reads
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MG_DIST_BACKEND="gloo",
               MG_DIST_REPORT="1")
    tmpw = tmp_path / "t_world2"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29671", os.path.join(ROOT, "tests", "dist_bam_reads.py"), str(bm), str(data),
                        "--temp_dir", str(tmpw), "--keep_temp_files", "--sketch_table", ref],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert (tmpw / "cmash_query_results.csv").read_bytes() == csv_ref
    shards = [(tmpw / ("shard_rank%d.txt" % q)).read_text().split() for q in (0, 1)]
    assert sum(int(s[0]) for s in shards) == len(reads) and all(int(s[0]) > 0 for s in shards)


def test_two_million_reads_at_the_default_grid(hip, oracle_lib, tmp_path):
    """2M reads of 150 bp as a BGZF BAM (unmapped, a tenth on the reverse strand) at the library's own grid and piece size."""
    rng = np.random.default_rng(18)
    gb, go = util.random_genomes(rng, 6, 20000)
    n, L = 2_000_000, 150
    start = rng.integers(0, int(go[-1]) - L, size=n)
    reads = gb[start[:, None] + np.arange(L)]
    m = rng.random(reads.shape) < 0.01
    reads[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(m.sum()))
    rev = rng.random(n) < 0.1
    code = np.zeros(256, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = [1, 2, 4, 8]
    stored = reads.copy()
    stored[rev] = np.frombuffer(b"TGCA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), reads[rev][:, ::-1])]
    c = code[stored]
    packed = (c[:, 0::2] << 4) | c[:, 1::2]
    # one record: block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen, "r%07d\0",
    # SEQ, QUAL (absent)
    name = 9
    size = 4 + 32 + name + L // 2 + L
    rec = np.zeros((n, size), np.uint8)
    rec[:, 0:4] = np.frombuffer(np.array([size - 4], "<u4").tobytes(), np.uint8)
    rec[:, 4:12] = 0xFF
    rec[:, 12] = name
    rec[:, 14:16] = np.frombuffer(np.array([4680], "<u2").tobytes(), np.uint8)
    rec[:, 18] = np.where(rev, 4 | 0x10, 4)
    rec[:, 20:24] = np.frombuffer(np.array([L], "<u4").tobytes(), np.uint8)
    rec[:, 24:32] = 0xFF
    digits = np.frombuffer(b"".join(b"r%07d\0" % i for i in range(0, 1)), np.uint8)  # (layout check)
    assert digits.size == name
    num = np.arange(n)
    rec[:, 36] = ord("r")
    for d in range(7):
        rec[:, 37 + d] = ord("0") + (num // 10 ** (6 - d)) % 10
    rec[:, 45:45 + L // 2] = packed
    rec[:, 45 + L // 2:] = 0xFF
    hdr = b"BAM\x01" + np.array([0, 0], "<i4").tobytes()
    p = tmp_path / "big.bam"
    p.write_bytes(bamgen.bgzf(hdr + rec.tobytes(), level=1))
    del rec, stored, packed, c
    rb = reads.reshape(-1)
    ro = (np.arange(n + 1, dtype=np.uint64) * L)
    r = hip.reads_from_bam_file(str(p))
    b, o = r.download()
    r.free()
    assert np.array_equal(o, ro) and np.array_equal(b, rb)
    h, khi, klo, go_ = hip.sketch_genomes_kmers(gb, go, 31, 300)
    table = hip.refdb_build(h, khi, klo, go_, [21, 31])
    want_table = oracle_lib.refpipe_build(h, khi, klo, go_, [21, 31])
    table.index_kmers()
    kc = table.kmer_counts()
    st = hip.count_stream(kc)
    st.add_file(str(p), "bam")
    st.free()
    want, seen = oracle_lib.refpipe_count_kmers(rb, ro, 31, want_table["kmer_hi"], want_table["kmer_lo"], cs=3)
    assert np.array_equal(kc.download(), want) and kc.stats()["kmers"] == seen and want.sum() > 0
    kc.free()
    table.free()
