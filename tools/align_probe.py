"""The device aligner (--aligner device; metalign_amd/align.py is the definition) on a shape a user would run: synthetic 150-base
reads with 1 % substitutions (metalign_amd/synth.py, seeded) against genomes of 5 Mbase.  The index build and, per batch of reads,
seeding, sort / unique, extension and selection are timed with device events (the library's own: mg_prof_*), after a warm-up batch.
Prints one JSON line: reads / s, candidates per read, the kernels' times.

    python tools/align_probe.py [--reads 10000000] [--genomes 100] [--genome_len 5000000] [--batch 2000000]

For the kernels' own times take, in a run of its own, `rocprofv3 --kernel-trace --stats -- python tools/align_probe.py ...`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("align_index", "align_seed", "align_unique", "align_extend", "align_select")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genomes", type=int, default=100)
    ap.add_argument("--genome_len", type=int, default=5_000_000)
    ap.add_argument("--batch", type=int, default=2_000_000, help="reads per call of mg_align_reads_dev")
    ap.add_argument("--present", type=int, default=50, help="genomes the reads are drawn from")
    ap.add_argument("--knob", action="append", default=[])
    args = ap.parse_args()
    from metalign_amd import _hip, align, synth
    from metalign_amd._hip import Hip
    hip = Hip.get(0)
    for kv in args.knob:
        k, v = kv.split("=")
        _hip.debug_set(k, int(v))
    p = align.params()
    t0 = time.time()
    gb, go = synth.make_genomes(args.genomes, args.genome_len)
    rb, ro, src = synth.make_reads(gb, go, args.reads, npresent=args.present)
    names = ["g%d" % g for g in range(args.genomes)]
    # the reference as the FASTA the aligner is given: one record per genome, one line each
    text = np.empty(int(go[-1]) + sum(len(n) + 3 for n in names), dtype=np.uint8)
    at = 0
    for g, name in enumerate(names):
        head = np.frombuffer(b">" + name.encode() + b"\n", dtype=np.uint8)
        seq = gb[int(go[g]):int(go[g + 1])]
        text[at:at + head.size] = head
        text[at + head.size:at + head.size + seq.size] = seq
        text[at + head.size + seq.size] = 10
        at += head.size + seq.size + 1
    made = time.time() - t0
    d_text, acc = hip.array(text), hip.acc_index(names)
    ref = hip.refseq_parse(d_text.ptr, text.size, acc, np.full(args.genomes, args.genome_len, dtype=np.uint64))
    d_text.free()
    acc.free()
    hip.prof_enable(True)
    hip.prof_reset()
    t0 = time.perf_counter()
    index = hip.align_index(ref, p.k, p.w)
    hip.sync()
    index_wall = time.perf_counter() - t0
    out = dict(reads=args.reads, genomes=args.genomes, genome_len=args.genome_len, batch=args.batch, params=p._asdict(),
               make_inputs_s=round(made, 1), index_wall_ms=round(index_wall * 1e3, 1), index_ms=round(hip.prof_get("align_index")[1], 3),
               index_entries=index.stats()[0], index_unique_keys=index.stats()[1])
    d_b = hip.array(np.concatenate([rb, np.zeros(64, np.uint8)]))
    d_o = hip.array(ro)

    def run(first, n):  # (the offsets are absolute: a batch is a window of them over the same bases)
        batch, stats = hip.align_reads_dev(index, d_b.ptr, d_o.ptr + 8 * first, n, p, placed=True, edited=True, based=True)
        batch.free()
        return stats

    run(0, min(args.batch, args.reads))  # warm-up: the pool's blocks and the sort's storage exist afterwards
    hip.sync()
    hip.prof_reset()
    total = np.zeros(5, dtype=np.int64)
    t0 = time.perf_counter()
    for first in range(0, args.reads, args.batch):
        total += np.asarray(run(first, min(args.batch, args.reads - first)))
    hip.sync()
    wall = time.perf_counter() - t0
    st = align.Stats(*total.tolist())
    ms = {f: round(hip.prof_get(f)[1], 3) for f in FAMILIES[1:]}
    out.update(stats=st._asdict(), wall_ms=round(wall * 1e3, 1), reads_per_s=round(args.reads / wall), device_ms=ms,
               candidates_per_read=round(st.candidates / max(st.reads, 1), 3), extend_candidates_per_s=round(st.candidates / max(ms["align_extend"], 1e-9) * 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
