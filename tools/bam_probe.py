"""BAM against BGZF SAM of the same alignments, in one process (DESIGN.md §4 "Ingest", BAM).

Writes N alignment records (150 bp reads, a primary and two secondaries each, from a seeded generator) as a BGZF SAM and as a
BAM, then times:
  * file -> records through mg_sam_stream_file and mg_bam_stream_file (the files warm in the page cache; best of --reps), with the
    device inflater (the default) and, with --host_inflate, the host readers;
  * mg_bam_tokenize_dev alone on the inflated BAM record stream resident in HBM (the boundary walk + stitch + decode + emit),
    in records/s and GB/s of inflated BAM.
The unit of --unit reads is generated once and repeated (its BGZF members too), so writing 10^7 records takes seconds.
Kernel times: run the same command under `rocprofv3 --kernel-trace --stats -- python tools/bam_probe.py ...`.

    python tools/bam_probe.py --records 10000000 --out profiles/r07/bam_probe.txt
"""
import argparse
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bamgen  # noqa: E402
import samgen  # noqa: E402
from metalign_amd import _hip  # noqa: E402


def unit_lines(nreads, accs, seed):
    rng = random.Random(seed)
    out = []
    for r in range(nreads):
        k = rng.randrange(100, 151)
        cig = "150M" if k == 150 else "%dM%dS" % (k, 150 - k)
        seq = samgen._seq(rng, 150)
        out.append(samgen._line("read%d" % r, rng.choice((0, 16)), rng.choice(accs), cig, seq, k & 7))
        for _ in range(2):
            out.append(samgen._line("read%d" % r, 256, rng.choice(accs), cig, "*", 1))
    return out


def members(data):
    return bamgen.bgzf(data, eof=False, level=1)


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--unit", type=int, default=50_000, help="reads generated once and repeated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host_inflate", action="store_true")
    ap.add_argument("--dir", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    _, accs, _ = samgen.make_dbinfo()
    lines = unit_lines(a.unit, accs, 1)
    rep = max(1, -(-a.records // len(lines)))
    data, hdr, names = bamgen.encode(lines)
    tmp = a.dir or tempfile.mkdtemp(prefix="bam_probe_")
    sam_p, bam_p = os.path.join(tmp, "x.sam.gz"), os.path.join(tmp, "x.bam")
    with open(sam_p, "wb") as fh:
        m = members("".join(lines).encode())
        for _ in range(rep):
            fh.write(m)
        fh.write(bamgen.EOF_BLOCK)
    with open(bam_p, "wb") as fh:
        fh.write(members(data[:hdr]))
        m = members(data[hdr:])
        for _ in range(rep):
            fh.write(m)
        fh.write(bamgen.EOF_BLOCK)
    n = len(lines) * rep
    sam_text = sum(len(x) for x in lines) * rep
    bam_bytes = (len(data) - hdr) * rep
    hip = _hip.Hip.get(0)
    if a.host_inflate:
        hip.inflate_config(on=0)
    acc_names = ["Unmapped"] + list(accs)
    idx = hip.acc_index(acc_names)
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    say("records %d (%d reads x 3), unit %d reads x %d" % (n, n // 3, a.unit, rep))
    say("BGZF SAM: %.3f GB compressed, %.3f GB text" % (os.path.getsize(sam_p) / 1e9, sam_text / 1e9))
    say("BAM:      %.3f GB compressed, %.3f GB inflated records" % (os.path.getsize(bam_p) / 1e9, bam_bytes / 1e9))
    say("inflater: %s" % ("host readers" if a.host_inflate else "device (k_inflate)"))

    def stream(fn, path):
        b = fn(path, idx)
        assert b.count == n, (b.count, n)
        b.free()

    t_sam = best(lambda: stream(hip.sam_stream_file, sam_p), a.reps)
    t_bam = best(lambda: stream(hip.bam_stream_file, bam_p), a.reps)
    say("file -> records  BGZF SAM  %.3f s  %.1f M records/s" % (t_sam, n / t_sam / 1e6))
    say("file -> records  BAM       %.3f s  %.1f M records/s" % (t_bam, n / t_bam / 1e6))
    # the record stream resident: the boundary + decode kernels (and the shared emit) alone
    stream_bytes = np.frombuffer(data[hdr:] * rep, dtype=np.uint8)
    refmap = np.array([acc_names.index(x) if x in acc_names else -1 for x in names], dtype=np.int32)
    d = hip.array(stream_bytes)

    def tok():
        b, used = hip.bam_tokenize_dev(d.ptr, stream_bytes.size, refmap, idx)
        assert b.count == n and used == stream_bytes.size
        b.free()

    tok()
    t_k = best(tok, a.reps)
    say("resident BAM -> records (mg_bam_tokenize_dev)  %.4f s  %.1f M records/s  %.1f GB/s of inflated BAM"
        % (t_k, n / t_k / 1e6, stream_bytes.size / t_k / 1e9))
    d.free()
    idx.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(report) + "\n")
    if not a.dir:
        for p in (sam_p, bam_p):
            os.unlink(p)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
