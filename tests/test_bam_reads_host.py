"""BAM READS files for stages A / B, where there is no GPU.

The read logic of the device (metalign_amd/csrc/mg_bam_core.h: seq_kept / kept_len / seq_span / seq_base) compiled for the HOST
(tests/host_bam_reads_check.cpp) must give back the reads a generated BAM was built from (tests/bamreads.py) — every nibble code,
odd lengths, both strands, records that are not reads skipped — without a load outside the record.  Then the pure-Python rendering
(bam.fastq_records) on the same streams, and the command lines (library stubbed): a BAM is taken by its content, the --input_type
choices stay, the streamed path asks for format 'bam', stage C gets a FASTQ and the profile keeps the BAM's name."""
import os
import struct
import subprocess

import pytest

import bamgen
import bamreads
from metalign_amd import bam, cli
from metalign_amd import map_and_profile as mapper
from metalign_amd import metalign
from metalign_amd import select_db as select

HERE = os.path.dirname(os.path.abspath(__file__))
CODES = "=ACMGRSVTWYHKDBN"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bamreads") / "host_bam_reads_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-o", out, os.path.join(HERE, "host_bam_reads_check.cpp")])
    return out


def _run(exe, tmp_path, stream, n_ref):
    p = tmp_path / "in.bin"
    p.write_bytes(struct.pack("<IQ", n_ref, len(stream)) + stream)
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.decode().splitlines()
    chain = lines[0].split()
    assert chain[0] == "chain" and int(chain[2]) == len(stream) and chain[3] == "0", lines[0]
    reads = []
    for ln in lines[1:-1]:
        tag, n, s = ln.split(" ")
        assert tag == "read"
        reads.append("" if s == "-" else s)
        assert len(reads[-1]) == int(n)
    kept = lines[-1].split()
    assert kept[0] == "kept" and int(kept[1]) == len(reads) and int(kept[2]) == sum(len(s) for s in reads)
    return reads


def _code_reads():
    """Every code at every place: odd and even lengths 1..35, each read also as its reverse complement."""
    reads = []
    for n in range(1, 36):
        for shift in range(0, 16, 5):
            s = "".join(CODES[(shift + 7 * i) % 16] for i in range(n))
            reads += [s, bamreads.revcomp(s)]
    return reads + [""]


def test_generated_bam_gives_back_its_reads(exe, tmp_path):
    reads, _, _ = bamreads.make_reads(seed=3, ntiles=30, nlong=2)
    _, stream, n_ref = bamreads.bam_bytes(reads, seed=4, bgzf=False)
    got = _run(exe, tmp_path, stream, n_ref)
    assert len(got) == len(reads) > 1900
    assert got == reads
    assert max(len(s) for s in reads) >= 15000 and "" in reads


def test_every_nibble_code_odd_lengths_and_both_strands(exe, tmp_path):
    reads = _code_reads()
    assert {c for s in reads for c in s} == set(CODES)
    _, stream, n_ref = bamreads.bam_bytes(reads, seed=5, bgzf=False)
    assert _run(exe, tmp_path, stream, n_ref) == reads
    # mapped on the reverse strand, one record each: the stored SEQ is the reverse complement, the read comes back as it was
    lines = ["@SQ\tSN:g0\tLN:100\n"] + ["q%d\t16\tg0\t1\t60\t%dM\t*\t0\t0\t%s\t*\n" % (i, len(s), bamreads.revcomp(s))
                                       for i, s in enumerate(reads) if s]
    data, hdr, names = bamgen.encode(lines)
    assert _run(exe, tmp_path, data[hdr:], len(names)) == [s for s in reads if s]


def test_records_that_are_not_reads_are_skipped(exe, tmp_path):
    sam = ["@SQ\tSN:g0\tLN:100\n",
           "a\t0\tg0\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\n",
           "a\t256\tg0\t1\t60\t3M\t*\t0\t0\tTTT\t*\n",
           "a\t2048\tg0\t1\t60\t3M\t*\t0\t0\tGGG\t*\n",
           "a\t2304\tg0\t1\t60\t3M\t*\t0\t0\tCCC\t*\n",
           "b\t1540\t*\t0\t0\t*\t*\t0\t0\tAC\t*\n",   # unmapped, duplicate, QC-fail: a read
           "c\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"]      # SEQ '*': an empty read
    data, hdr, names = bamgen.encode(sam)
    assert _run(exe, tmp_path, data[hdr:], len(names)) == ["ACGT", "AC", ""]


def _records(blob):
    lines = blob.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:].decode(), lines[i + 1].decode(), lines[i + 3].decode()) for i in range(0, len(lines) - 1, 4)]


def test_host_fastq_rendering_on_the_same_streams(tmp_path):
    for reads, seed in ((bamreads.make_reads(seed=6, ntiles=12, nlong=1)[0], 7), (_code_reads(), 8)):
        p = tmp_path / ("x%d.bam" % seed)
        p.write_bytes(bamreads.bam_bytes(reads, seed=seed, block=3000)[0])
        got = _records(b"".join(bam.fastq_records(str(p))))
        assert [s for _, s, _ in got] == reads
        assert [q for q, _, _ in got] == ["r%d" % i for i in range(len(reads))]
        assert all(len(q) == len(s) and set(q) <= {"I", '"'} for _, s, q in got)
    # QUAL is reversed with the bases on the reverse strand; an absent QUAL is quality 1
    lines = ["@SQ\tSN:g0\tLN:100\n", "q\t16\tg0\t1\t60\t3M\t*\t0\t0\tAAC\t!#%\n", "u\t4\t*\t0\t0\t*\t*\t0\t0\tMR\t*\n"]
    p = tmp_path / "q.bam"
    p.write_bytes(bamgen.sam_to_bam("".join(lines)))
    assert _records(b"".join(bam.fastq_records(str(p)))) == [("q", "GTT", "%#!"), ("u", "MR", '""')]
    # a cut file: an error naming it
    cut = tmp_path / "cut.bam"
    cut.write_bytes(bamgen.encode(lines)[0][:-5])
    with pytest.raises(ValueError, match="cut.bam"):
        list(bam.fastq_records(str(cut)))


def test_a_bam_is_taken_by_its_content_and_the_choices_stay(tmp_path):
    reads = ["ACGT", "GGA"]
    for name, bgzf in (("x.bam", True), ("x.fq", True), ("plain.fastq", False)):
        p = tmp_path / name
        p.write_bytes(bamreads.bam_bytes(reads, bgzf=bgzf)[0])
        for given in ("AUTO", "fastq", "fasta"):
            assert cli.reads_kind(str(p), given) == "bam"
    fq = tmp_path / "y.fq"
    fq.write_bytes(bamreads.fastq_text(reads))
    assert cli.reads_kind(str(fq), "AUTO") == "fastq" and cli.reads_kind(str(fq), "fasta") == "fasta"
    for tool in ("metalign", "select_db"):
        act = [a for a in cli.parser_for(tool)._actions if a.dest == "input_type"][0]
        assert act.choices == ["fastq", "fasta", "AUTO"]


class _FakeStream:
    def __init__(self, log):
        self.log, self.nbases = log, 0

    def add_file(self, path, fmt, **kw):
        self.log.append((path, fmt))

    def finish(self):
        return []

    def free(self):
        pass


class _FakeHip:
    def __init__(self):
        self.log = []

    def sketch_stream(self, *a):
        return _FakeStream(self.log)

    def count_stream(self, counts):
        return _FakeStream(self.log)


def _data_dir(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    (data / "db_info.txt").write_text("Accesion\tLength\tTaxID\tLineage\tTaxID_Lineage\n")
    return data


def test_select_db_streams_a_bam_as_format_bam(tmp_path, monkeypatch):
    p = tmp_path / "reads.fq"  # (a BAM whatever its name)
    p.write_bytes(bamreads.bam_bytes(["ACGTACGT", "TTTT"])[0])
    fake = _FakeHip()
    assert select.stream_reads_file(fake, str(p), "bam", [21], [1], 0, [None]) == []
    assert fake.log == [(str(p), "bam")]
    assert select.reads_format("bam") == "bam" and select.reads_format("fasta") == "fasta_ml"
    assert select.expected_bases(str(p), "bam") > 0
    seen = {}

    def fake_steps(args):
        seen["kind"] = args.input_type
        with open(args.temp_dir + "cmash_query_results.csv", "w") as fh:
            fh.write(",k=21\n")
    monkeypatch.setattr(select, "run_sketch_steps", fake_steps)
    monkeypatch.setattr(select, "make_db_and_dbinfo", lambda *a: None)
    data = _data_dir(tmp_path)
    args = select.select_parseargs([str(p), str(data), "--input_type", "fastq", "--temp_dir", str(tmp_path / "t")])
    select.select_main(args)
    assert seen["kind"] == "bam"


def test_metalign_hands_stage_c_a_fastq_and_keeps_the_sample_id(tmp_path, monkeypatch):
    reads = ["ACGTNACGT", "", "GATTACA"]
    p = tmp_path / "sample.bam"
    p.write_bytes(bamreads.bam_bytes(reads, seed=2)[0])
    seen = {}
    def fake_select(args):
        seen["kind"] = args.input_type
        os.makedirs(args.temp_dir, exist_ok=True)  # (what select_main does first)
    monkeypatch.setattr(metalign.select, "select_main", fake_select)

    def fake_map(args):
        seen["infiles"], seen["type"] = list(args.infiles), args.input_type
        seen["fq"] = open(args.infiles[0], "rb").read()
        mapper.write_results(args, [[] for _ in mapper.RANKS])
    monkeypatch.setattr(metalign.mapper, "map_main", fake_map)
    data = _data_dir(tmp_path)
    out = tmp_path / "prof.tsv"
    tmpd = tmp_path / "tmp"
    metalign.main([str(p), str(data), "--temp_dir", str(tmpd), "--output", str(out), "--keep_temp_files"])
    assert seen["kind"] == "bam" and seen["type"] == "fastq"
    assert seen["infiles"] == [str(tmpd) + "/reads_from_bam.fq"] and os.path.exists(seen["infiles"][0])
    assert [s for _, s, _ in _records(seen["fq"])] == reads
    assert out.read_text().startswith("@SampleID:%s\n" % p)
    # --sampleID given: kept as given; without --keep_temp_files the FASTQ goes with the temporary directory
    tmp2 = tmp_path / "tmp2"
    metalign.main([str(p), str(data), "--temp_dir", str(tmp2), "--output", str(out), "--sampleID", "s9"])
    assert out.read_text().startswith("@SampleID:s9\n") and not tmp2.exists()
