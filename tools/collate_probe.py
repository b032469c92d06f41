"""What collating by read costs next to the stream it rides on.

The >= 2 M-record BAM of tests/test_gpu_bam.py::test_full_size_bam_equals_bgzf_sam's generator (6 700 reads of 40 bp, a primary and
two secondaries each, the record stream x 100) with its RECORDS shuffled — what a coordinate sort does to a read's alignments —
through mg_bam_stream_file (`--collate never`) and through mg_bam_stream_file_collated, the file warm in the page cache, best of
--reps; and the collation alone on the keyed batch resident in HBM (knob collate_defer).

    python tools/collate_probe.py --out profiles/collate_probe.txt
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


def best(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rep", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    _, accs, _ = samgen.make_dbinfo()
    rng = random.Random(4)
    lines = []
    for r in range(6700):
        k = rng.randrange(20, 41)
        cig = "40M" if k == 40 else "%dM%dS" % (k, 40 - k)
        lines.append(samgen._line("r%d" % r, rng.choice((0, 16)), rng.choice(accs), cig, samgen._seq(rng, 40), k & 7))
        for _ in range(2):
            lines.append(samgen._line("r%d" % r, 256, rng.choice(accs), cig, "*", 1))
    data, hdr, _ = bamgen.encode(lines)
    recs, p = [], hdr
    while p < len(data):
        q = p + 4 + int.from_bytes(data[p:p + 4], "little")
        recs.append(data[p:q])
        p = q
    order = list(range(len(recs))) * a.rep
    rng.shuffle(order)
    n = len(order)
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")

    hip = _hip.Hip.get(0)
    idx = hip.acc_index(["Unmapped"] + list(accs))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "shuffled.bam")
        with open(path, "wb") as fh:
            fh.write(bamgen.bgzf(data[:hdr] + b"".join(recs[i] for i in order), level=1))
        say("%d records, %d names, BAM of %.1f MB" % (n, 6700, os.path.getsize(path) / 1e6))

        def stream(collate):
            b = hip.bam_stream_file(path, idx, collate=collate)
            assert b.count == n
            b.free()

        stream(False), stream(True)  # (warm: the page cache, the scratch buffers, the pool)
        t_never = best(lambda: stream(False), a.reps)
        t_coll = best(lambda: stream(True), a.reps)
        say("mg_bam_stream_file            %.4f s  %.1f M records/s" % (t_never, n / t_never / 1e6))
        say("mg_bam_stream_file_collated   %.4f s  %.1f M records/s  (+ %.4f s, x %.2f)" % (t_coll, n / t_coll / 1e6, t_coll - t_never,
                                                                                           t_coll / t_never))
        _hip.debug_set("collate_defer", 1)
        ts = []
        for _ in range(a.reps):
            b = hip.bam_stream_file(path, idx, collate=True)
            hip.sync()
            t0 = time.perf_counter()
            b.collate()
            ts.append(time.perf_counter() - t0)
            heads = int((b.download()["ref_new"] >> np.uint32(31)).sum())
            b.free()
        _hip.debug_set(None)
        say("mg_sam_batch_collate_dev      %.4f s  %.1f M records/s  (%d reads)" % (min(ts), n / min(ts) / 1e6, heads))
        say("beside the 16 B records: 16 B of key per record until collated; during the call 4 x 8 B sort arrays, the radix sort's own "
            "storage and the 16 B regrouped copy")
    idx.free()
    if out:
        out.close()


if __name__ == "__main__":
    main()
