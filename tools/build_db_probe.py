"""What reading the organism files costs `build_db`, on the host and on the device (DESIGN.md §8, row f2').

Synthetic genomes (metalign_amd/synth.py: iid ACGT) written as FASTA with 70-column lines, every other file `.gz`; by default
2 000 files x 2 Mb.  The same files, warm in the page cache, go through `build_db --ingest host` and `--ingest device` (the stock
four k, n = 1000); the two table directories are compared byte for byte.  For the device path the split is printed too: the reader
threads' read + inflate (summed over the threads), the uploader queueing copies, next() waiting for a batch to be up, the parse,
and the sketching (what is left of the wall time is Python, the filters and the table files).

    python tools/build_db_probe.py --out profiles/r07/build_db_ingest.txt
"""
import argparse
import filecmp
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metalign_amd import _hip, build_db, synth  # noqa: E402

THREADS = 16


def write_files(d, nfiles, length, width):
    """-> paths.  Genome i: two records (a 'N' joins them), `width`-column lines; odd i: gzip (level 1: what costs here is reading)."""
    def one(i):
        bases, _ = synth.make_genomes(1, length, seed=synth.SEED + 17 * i)
        cut = length // 3
        parts = []
        for r, rec in enumerate((bases[:cut], bases[cut:])):
            full = len(rec) // width * width
            body = np.full((full // width, width + 1), 10, dtype=np.uint8)
            body[:, :width] = rec[:full].reshape(-1, width)
            parts.append(b">genome%d_contig%d synthetic\n" % (i, r) + body.tobytes() + (rec[full:].tobytes() + b"\n" if full < len(rec) else b""))
        text = b"".join(parts)
        p = os.path.join(d, "taxid_%d_genomic.fna%s" % (i, ".gz" if i & 1 else ""))
        with open(p, "wb") as fh:
            if i & 1:
                c = zlib.compressobj(1, zlib.DEFLATED, 31)
                fh.write(c.compress(text) + c.flush())
            else:
                fh.write(text)
        return p
    with ThreadPoolExecutor(THREADS) as ex:
        return sorted(ex.map(one, range(nfiles)))


def timed_sketchers(hip, acc):
    """The Hip instance's genome sketch calls wrapped so that their wall time adds up in acc['sketch']."""
    saved = {}
    for name in ("sketch_genomes", "sketch_genomes_dev", "sketch_genomes_prefix", "sketch_genomes_prefix_dev",
                 "sketch_genomes_kmers", "sketch_genomes_kmers_dev"):
        fn = getattr(hip, name)
        saved[name] = fn

        def wrapped(*a, _fn=fn, **kw):
            t0 = time.perf_counter()
            try:
                return _fn(*a, **kw)
            finally:
                acc["sketch"] += time.perf_counter() - t0
        setattr(hip, name, wrapped)
    return saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=70)
    ap.add_argument("--ks", default="30,40,50,60")
    ap.add_argument("-n", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    hip = _hip.Hip.get(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "organisms")
        os.mkdir(src)
        t0 = time.perf_counter()
        paths = write_files(src, a.files, a.length, a.width)
        nbytes = sum(os.path.getsize(p) for p in paths)
        say("build_db ingest probe on %s: %d files x %d bases, %d-column lines, every other file .gz (level 1); %.2f GB on disk, written in %.1f s"
            % (hip.device_name(), a.files, a.length, a.width, nbytes / 1e9, time.perf_counter() - t0))
        say("k = %s, n = %d, reader threads = %d, files warm in the page cache" % (a.ks, a.n, THREADS))
        for p in paths:  # warm
            with open(p, "rb") as fh:
                while fh.read(1 << 24):
                    pass
        took = {}
        for ingest in ("device", "host"):
            acc = {"sketch": 0.0}
            saved = timed_sketchers(hip, acc)
            try:
                t0 = time.perf_counter()
                build_db.build(paths, os.path.join(d, ingest), ks, a.n, ingest=ingest)
                took[ingest] = time.perf_counter() - t0
            finally:
                for name, fn in saved.items():
                    setattr(hip, name, fn)
            say("--ingest %-6s  %8.2f s   (of it in the sketch calls: %.2f s)" % (ingest, took[ingest], acc["sketch"]))
            if ingest == "device":
                st = hip.genome_stream_stats
                say("   device split: read+inflate %.2f thread-s (/%d threads = %.2f s), upload queueing %.2f s, waiting for a batch %.2f s, "
                    "parse %.2f s, sketch %.2f s; %.2f GB of text went up; host-parsed files: %d"
                    % (st["read_inflate_s"], THREADS, st["read_inflate_s"] / THREADS, st["upload_s"], st["wait_s"], st["parse_s"], acc["sketch"],
                       st["text_bytes"] / 1e9, hip.genomes_host_parsed))
        names = sorted(os.listdir(os.path.join(d, "host")))
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(d, "host"), os.path.join(d, "device"), names, shallow=False)
        say("tables identical: %s (%d files)" % ("yes" if not mismatch and not errors and names == sorted(os.listdir(os.path.join(d, "device"))) else "NO", len(names)))
        say("host / device = %.2fx" % (took["host"] / took["device"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
