"""The device aligner (--aligner device; metalign_amd/align.py is the definition) on a shape a user would run: synthetic 150-base
reads with 1 % substitutions (metalign_amd/synth.py, seeded) against genomes of 5 Mbase.  The index build and, per batch of reads,
seeding, sort / unique, extension, mate rescue (--pairs), gapped refinement (--band) and selection are timed with device events (the library's own: mg_prof_*), after a warm-up batch.
Prints one JSON line: reads / s, candidates per read, the kernels' times.

    python tools/align_probe.py [--reads 10000000] [--genomes 100] [--genome_len 5000000] [--batch 2000000] [--band 8 --indel_rate 0.1]
                                [--pairs --insert 300,600 --unseedable 0.1 --max_insert 1000 --rescue 2]

--indel_rate F: that share of the reads (every round(1 / F)-th) carries one planted insertion or deletion, in turn, of 1 .. band bases.
--pairs: the reads are interleaved pairs (--align_pairs interleaved): two mates of 150 bases from the ends of fragments whose length
is uniform in --insert LO,HI, every other pair with mate 1 on the reverse strand, 1 % substitutions.  --unseedable F: that share of
the pairs (every round(1 / F)-th) has a substitution at every 12th base of mate 2, which leaves it no 15-mer: only rescue finds it.
The ABI does not report the rescue tasks; the probe gives the rescued candidates, and from them a LOWER bound of the columns
k_al_rescue scanned (each rescued mate took at least one window of max_insert - 149 diagonals by 150 columns).

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

FAMILIES = ("align_index", "align_seed", "align_unique", "align_extend", "align_rescue", "align_refine", "align_select")


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


def make_pairs(gb, go, npairs, present, insert, unseedable_every, sub=0.01):
    """Interleaved pairs -> (bases, offsets): see the module's text."""
    rng = np.random.default_rng(7)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    lens = np.diff(go).astype(np.int64)
    g = rng.integers(0, present, size=npairs)
    F = rng.integers(insert[0], insert[1] + 1, size=npairs)
    start = go[g].astype(np.int64) + (rng.random(npairs) * (lens[g] - F)).astype(np.int64)
    col = np.arange(150, dtype=np.int64)
    sites = np.arange(5, 150, 12)
    out = np.empty((npairs, 2, 150), dtype=np.uint8)
    for lo in range(0, npairs, 1 << 17):  # (in slices: the index arrays are eight times the bases)
        st, fl = start[lo:lo + (1 << 17)], F[lo:lo + (1 << 17)]
        fwd = gb[st[:, None] + col[None, :]]
        rev = comp[gb[(st + fl - 1)[:, None] - col[None, :]]]
        for m in (fwd, rev):  # substitutions: the complementary base
            hit = rng.random(m.shape) < sub
            m[hit] = comp[m[hit]]
        flip = (np.arange(lo, lo + st.size) % 2 == 1)[:, None]
        m1, m2 = np.where(flip, rev, fwd), np.where(flip, fwd, rev)
        if unseedable_every:
            rows = np.nonzero(np.arange(lo, lo + st.size) % unseedable_every == 0)[0]
            m2[np.ix_(rows, sites)] = comp[m2[np.ix_(rows, sites)]]
        out[lo:lo + st.size, 0], out[lo:lo + st.size, 1] = m1, m2
    return out.reshape(-1), (np.arange(2 * npairs + 1, dtype=np.uint64) * 150)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genomes", type=int, default=100)
    ap.add_argument("--genome_len", type=int, default=5_000_000)
    ap.add_argument("--batch", type=int, default=2_000_000, help="reads per call of mg_align_reads_dev")
    ap.add_argument("--present", type=int, default=50, help="genomes the reads are drawn from")
    ap.add_argument("--band", type=int, default=0, help="--align_band: 0 leaves the aligner ungapped")
    ap.add_argument("--indel_rate", type=float, default=0.0, help="the share of reads with one planted indel of 1 .. band bases")
    ap.add_argument("--pairs", action="store_true", help="--align_pairs interleaved on synthetic interleaved pairs")
    ap.add_argument("--insert", default="300,600", help="--pairs: the fragment lengths, LO,HI")
    ap.add_argument("--unseedable", type=float, default=0.0, help="--pairs: the share of pairs whose mate 2 has a substitution at every 12th base")
    ap.add_argument("--max_insert", type=int, default=1000)
    ap.add_argument("--rescue", type=int, default=2)
    ap.add_argument("--knob", action="append", default=[])
    args = ap.parse_args()
    from metalign_amd import _hip, align, synth
    from metalign_amd._hip import Hip
    hip = Hip.get(0)
    for kv in args.knob:
        k, v = kv.split("=")
        _hip.debug_set(k, int(v))
    p, gp = align.params(), align.gap_params(args.band)
    pp = align.pair_params(1, args.max_insert, args.rescue) if args.pairs else None
    t0 = time.time()
    gb, go = synth.make_genomes(args.genomes, args.genome_len)
    if args.pairs:
        lo, hi = (int(x) for x in args.insert.split(","))
        rb, ro = make_pairs(gb, go, args.reads // 2, args.present, (lo, hi), max(1, round(1 / args.unseedable)) if args.unseedable > 0 else 0)
    else:
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
        if pp is None:
            batch, stats, refined = hip.align_reads_gapped_dev(index, d_b.ptr, d_o.ptr + 8 * first, n, p, gp, placed=True, edited=True, based=True)
            batch.free()
            return tuple(stats) + (refined, 0, 0)
        batch, stats, ps = hip.align_reads_paired_dev(index, d_b.ptr, d_o.ptr + 8 * first, n, p, gp, pp, placed=True, edited=True, based=True)
        batch.free()
        return tuple(stats) + tuple(ps)

    run(0, min(args.batch, args.reads))  # warm-up: the pool's blocks and the sort's storage exist afterwards
    hip.sync()
    hip.prof_reset()
    total = np.zeros(8, dtype=np.int64)
    t0 = time.perf_counter()
    for first in range(0, args.reads, args.batch):
        total += np.asarray(run(first, min(args.batch, args.reads - first)))
    hip.sync()
    wall = time.perf_counter() - t0
    st = align.Stats(*total[:5].tolist())
    ms = {f: round(hip.prof_get(f)[1], 3) for f in FAMILIES[1:]}
    out.update(gap=gp._asdict(), indel_rate=args.indel_rate, refined=int(total[5]), stats=st._asdict(), wall_ms=round(wall * 1e3, 1), reads_per_s=round(args.reads / wall), device_ms=ms,
               candidates_per_read=round(st.candidates / max(st.reads, 1), 3), extend_candidates_per_s=round(st.candidates / max(ms["align_extend"], 1e-9) * 1e3))
    if pp is not None:
        columns = int(total[6]) * max(args.max_insert - 149, 1) * 150
        out.update(pairs=pp._asdict(), insert=args.insert, unseedable=args.unseedable, rescued=int(total[6]), proper_pairs=int(total[7]),
                   rescue_columns_at_least=columns, rescue_columns_per_s_at_least=round(columns / max(ms["align_rescue"], 1e-9) * 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
