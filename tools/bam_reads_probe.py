"""BAM READS files against FASTQ of the same reads, stage A (k-mer identity counters), in one process (DESIGN.md §3 f4″).

Writes N seeded 150 bp reads (a unit generated once and repeated, with binned random qualities) as plain FASTQ, `.fq.gz` (BGZF),
BGZF BAM and uncompressed BAM (unmapped records, a tenth stored reverse-complemented with 0x10), then times each file -> the
stage-A counters through mg_sketch_stream_add_file (best of --reps, the files warm in the page cache), checks that every file
gives the same counters, and times mg_reads_parse_bam_prefix_dev alone on the record stream resident in HBM.
Kernel times: run the same command under `rocprofv3 --kernel-trace --stats -- python tools/bam_reads_probe.py ...` (a separate
run: the tracer changes the timings).

    python tools/bam_reads_probe.py --reads 10000000 --out profiles/r07/bam_reads_probe.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bamgen  # noqa: E402
from metalign_amd import _hip  # noqa: E402

L = 150
NAME = 9  # "r%07d\0"


def unit_reads(rng, gb, n):
    start = rng.integers(0, gb.size - L, size=n)
    reads = gb[start[:, None] + np.arange(L)]
    m = rng.random(reads.shape) < 0.01
    reads[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(m.sum()))
    qual = rng.choice(np.array([2, 11, 25, 37], np.uint8), size=reads.shape, p=[0.05, 0.1, 0.25, 0.6])
    return reads, qual


def fastq_unit(reads, qual):
    n = len(reads)
    head = np.frombuffer(b"".join(b"@r%07d\n" % i for i in range(n)), np.uint8).reshape(n, NAME + 1)
    rec = np.concatenate([head, reads, np.full((n, 3), [10, 43, 10], np.uint8), qual + 33, np.full((n, 1), 10, np.uint8)], axis=1)
    return rec.tobytes()


def bam_unit(rng, reads, qual):
    n = len(reads)
    rev = rng.random(n) < 0.1
    stored, q = reads.copy(), qual.copy()
    acgt = np.frombuffer(b"ACGT", np.uint8)
    stored[rev] = np.frombuffer(b"TGCA", np.uint8)[np.searchsorted(acgt, reads[rev][:, ::-1])]
    q[rev] = qual[rev][:, ::-1]
    code = np.zeros(256, np.uint8)
    code[acgt] = [1, 2, 4, 8]
    c = code[stored]
    size = 4 + 32 + NAME + L // 2 + L
    rec = np.zeros((n, size), np.uint8)
    rec[:, 0:4] = np.frombuffer(np.array([size - 4], "<u4").tobytes(), np.uint8)
    rec[:, 4:12] = 0xFF
    rec[:, 12] = NAME
    rec[:, 14:16] = np.frombuffer(np.array([4680], "<u2").tobytes(), np.uint8)
    rec[:, 18] = np.where(rev, 4 | 0x10, 4)
    rec[:, 20:24] = np.frombuffer(np.array([L], "<u4").tobytes(), np.uint8)
    rec[:, 24:32] = 0xFF
    rec[:, 36:45] = np.frombuffer(b"".join(b"r%07d\0" % i for i in range(n)), np.uint8).reshape(n, NAME)
    rec[:, 45:45 + L // 2] = (c[:, 0::2] << 4) | c[:, 1::2]
    rec[:, 45 + L // 2:] = q
    return rec.tobytes()


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--unit", type=int, default=100_000, help="reads generated once and repeated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="one file kind (fq, fq.gz, bam, ubam): for a kernel trace of that file alone")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    gb = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=4_000_000)
    reads, qual = unit_reads(rng, gb, a.unit)
    rep = max(1, -(-a.reads // a.unit))
    n = a.unit * rep
    fq_u, bam_u = fastq_unit(reads, qual), bam_unit(rng, reads, qual)
    hdr = b"BAM\x01" + np.array([0, 0], "<i4").tobytes()
    tmp = a.dir or tempfile.mkdtemp(prefix="bam_reads_probe_")
    files = {"fq": os.path.join(tmp, "x.fq"), "fq.gz": os.path.join(tmp, "x.fq.gz"), "bam": os.path.join(tmp, "x.bam"),
             "ubam": os.path.join(tmp, "x.ubam.bam")}
    kinds = [a.only] if a.only else list(files)
    units = {"fq": (b"", fq_u, False), "fq.gz": (b"", fq_u, True), "bam": (hdr, bam_u, True), "ubam": (hdr, bam_u, False)}
    for kd in kinds:
        head, unit, gz = units[kd]
        with open(files[kd], "wb") as fh:
            if gz:
                if head:
                    fh.write(bamgen.bgzf(head, eof=False, level=1))
                m = bamgen.bgzf(unit, eof=False, level=1)
            else:
                fh.write(head)
                m = unit
            for _ in range(rep):
                fh.write(m)
            if gz:
                fh.write(bamgen.EOF_BLOCK)
    hip = _hip.Hip.get(0)
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    say("reads %d x %d bp (unit %d x %d)" % (n, L, a.unit, rep))
    for kd in kinds:
        say("%-6s %.3f GB" % (kd, os.path.getsize(files[kd]) / 1e9))
    gbs = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=12 * 20000)
    gbs[:200000] = gb[:200000]  # (some genomes the reads come from: counters that are not all zero)
    go = (np.arange(13) * 20000).astype(np.uint64)
    ks = [21, 31]
    h, khi, klo, o = hip.sketch_genomes_kmers(gbs, go, ks[-1], 1000)
    table = hip.refdb_build(h, khi, klo, o, ks)
    table.index_kmers()
    ref = None
    for kd in kinds:
        fmt = "bam" if "bam" in kd else "fastq"
        out = {}

        def run():
            kc = table.kmer_counts()
            st = hip.count_stream(kc)
            st.add_file(files[kd], fmt)
            st.free()
            out["c"] = kc.download()
            kc.free()

        t = best(run, a.reps)
        if ref is None:
            ref = out["c"]
        same = np.array_equal(out["c"], ref)
        say("file -> stage-A counters  %-6s %.4f s  %.1f M reads/s  counters %s" % (kd, t, n / t / 1e6,
                                                                                  "equal" if same else "DIFFER"))
    table.free()
    if not a.only or a.only == "ubam":
        stream = np.frombuffer(bam_u * rep, dtype=np.uint8)
        d = hip.array(stream)

        def unpack():
            r, used = hip.parse_bam_reads_dev(d.ptr, stream.size, 0, final=True)
            assert r.count == n and used == stream.size
            r.free()

        unpack()
        t = best(unpack, a.reps)
        say("resident BAM records -> bases + offsets (mg_reads_parse_bam_prefix_dev)  %.4f s  %.1f GB/s of records"
            % (t, stream.size / t / 1e9))
        d.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(report) + "\n")
    if not a.dir:
        for kd in kinds:
            os.unlink(files[kd])
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
