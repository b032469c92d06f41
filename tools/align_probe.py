"""The device aligner (--aligner device; metalign_amd/align.py is the definition) on a shape a user would run: synthetic 150-base
reads with 1 % substitutions (metalign_amd/synth.py, seeded) against genomes of 5 Mbase.  The index build and, per batch of reads,
seeding, sort / unique, extension, gapped refinement (--band) and selection are timed with device events (the library's own: mg_prof_*), after a warm-up batch.
Prints one JSON line: reads / s, candidates per read, the kernels' times.

    python tools/align_probe.py [--reads 10000000] [--genomes 100] [--genome_len 5000000] [--batch 2000000] [--band 8 --indel_rate 0.1]

--indel_rate F: that share of the reads (every round(1 / F)-th) carries one planted insertion or deletion, in turn, of 1 .. band bases.

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

FAMILIES = ("align_index", "align_seed", "align_unique", "align_extend", "align_refine", "align_select")


def plant_indels(rb, ro, every, longest):
    """Every `every`-th read of 40 bases or more gets one indel of 1 .. longest bases 20 bases or more from its ends: a deletion
    (the bases go) and an insertion (random bases come) in turn -> (bases, offsets)."""
    rng = np.random.default_rng(5)
    lens = np.diff(ro).astype(np.int64)
    picks = np.arange(0, lens.size, every)
    picks = picks[lens[picks] >= 40 + longest]
    size = rng.integers(1, longest + 1, size=picks.size)
    at = (rng.random(picks.size) * (lens[picks] - 40 - size)).astype(np.int64) + 20
    delete = np.arange(picks.size) % 2 == 0
    # deletions: drop the bases; insertions: overwrite them with random ones and take as many off the read's end (the length stays)
    keep = np.ones(rb.size, dtype=bool)
    out = rb.copy()
    for r, a, g, is_del in zip(picks.tolist(), at.tolist(), size.tolist(), delete.tolist()):
        lo, hi = int(ro[r]), int(ro[r + 1])
        if is_del:
            keep[lo + a:lo + a + g] = False
        else:
            out[lo + a + g:hi] = rb[lo + a:hi - g]
            out[lo + a:lo + a + g] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=g)
    new_lens = lens.copy()
    new_lens[picks[delete]] -= size[delete]
    offs = np.zeros(lens.size + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(new_lens)
    return out[keep], offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genomes", type=int, default=100)
    ap.add_argument("--genome_len", type=int, default=5_000_000)
    ap.add_argument("--batch", type=int, default=2_000_000, help="reads per call of mg_align_reads_dev")
    ap.add_argument("--present", type=int, default=50, help="genomes the reads are drawn from")
    ap.add_argument("--band", type=int, default=0, help="--align_band: 0 leaves the aligner ungapped")
    ap.add_argument("--indel_rate", type=float, default=0.0, help="the share of reads with one planted indel of 1 .. band bases")
    ap.add_argument("--knob", action="append", default=[])
    args = ap.parse_args()
    from metalign_amd import _hip, align, synth
    from metalign_amd._hip import Hip
    hip = Hip.get(0)
    for kv in args.knob:
        k, v = kv.split("=")
        _hip.debug_set(k, int(v))
    p, gp = align.params(), align.gap_params(args.band)
    t0 = time.time()
    gb, go = synth.make_genomes(args.genomes, args.genome_len)
    rb, ro, src = synth.make_reads(gb, go, args.reads, npresent=args.present)
    if args.indel_rate > 0:
        rb, ro = plant_indels(rb, ro, max(1, round(1 / args.indel_rate)), max(args.band, 1))
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
        batch, stats, refined = hip.align_reads_gapped_dev(index, d_b.ptr, d_o.ptr + 8 * first, n, p, gp, placed=True, edited=True, based=True)
        batch.free()
        return tuple(stats) + (refined,)

    run(0, min(args.batch, args.reads))  # warm-up: the pool's blocks and the sort's storage exist afterwards
    hip.sync()
    hip.prof_reset()
    total = np.zeros(6, dtype=np.int64)
    t0 = time.perf_counter()
    for first in range(0, args.reads, args.batch):
        total += np.asarray(run(first, min(args.batch, args.reads - first)))
    hip.sync()
    wall = time.perf_counter() - t0
    st = align.Stats(*total[:5].tolist())
    ms = {f: round(hip.prof_get(f)[1], 3) for f in FAMILIES[1:]}
    out.update(gap=gp._asdict(), indel_rate=args.indel_rate, refined=int(total[5]), stats=st._asdict(), wall_ms=round(wall * 1e3, 1), reads_per_s=round(args.reads / wall), device_ms=ms,
               candidates_per_read=round(st.candidates / max(st.reads, 1), 3), extend_candidates_per_s=round(st.candidates / max(ms["align_extend"], 1e-9) * 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
