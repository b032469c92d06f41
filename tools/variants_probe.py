"""What --variants costs on the device.

Kernels: mg_variants_add_dev against mg_depth_add_dev and mg_coverage_add_dev on the same --records synthetic 150-base records, in
identity_probe's two mixes (95 % of the records on 5 of 500 accessions; spread evenly), and mg_variants_finish behind each.
Tokeniser: mg_sam_tokenize_dev_ex with MG_BATCH_PLACES against PLACES | BASES on the same resident SAM text of --lines lines
(tools/coverage_probe.py's file: one 150-base read per line).
End to end: map_and_profile over that text as a file without the flags and with --variants (--e2e alone runs at any commit: without
the flag it uses nothing this tool's other parts need; MG_PROBE_ROOT names the package to import; a flag the commit's parser does
not have is left out).  Best of --reps for the kernels and the tokeniser; for the end-to-end runs every repeat is printed.

    python tools/variants_probe.py --out profiles/r12/variants_probe.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_probe as cp  # noqa: E402  (puts the package's root on sys.path)

from metalign_amd import _hip  # noqa: E402

NACC, ACC_LEN, READ = cp.NACC, cp.ACC_LEN, cp.READ


def end_to_end(say, d, reps):
    import argparse as ap
    from metalign_amd import cli, map_and_profile as mp

    def run(flags):
        args = ap.Namespace(infiles=[os.path.join(d, "probe.sam")], data="data/", db="NONE", dbinfo=os.path.join(d, "db_info.txt"),
                            input_type="sam", length_normalize=False, low_mem=False, min_abundance=10 ** -4, rank_renormalize=False,
                            output=os.path.join(d, "out.cami"), pct_id=0.5, no_quantify_unmapped=False, read_cutoff=1, sampleID="probe",
                            threads=4, verbose=False)
        for flag in flags:
            setattr(args, flag, os.path.join(d, flag + ".tsv"))
        t0 = time.perf_counter()
        mp.map_main(args)
        return time.perf_counter() - t0
    known = {a.dest for a in cli.parser_for("map_and_profile")._actions}  # (which flags the commit under test has)
    for label, flags in (("no flag", ()), ("--variants", ("variants",))):
        if not set(flags) <= known:
            continue
        run(flags)
        t = [run(flags) for _ in range(reps)]
        say("map_and_profile end to end, %-12s %s ms   (median %.2f, spread %.2f)"
            % (label, " ".join("%.2f" % (x * 1e3) for x in t), float(np.median(t)) * 1e3, (max(t) - min(t)) * 1e3))


def kernels(say, hip, rng, a):
    n = a.records
    lengths = np.full(NACC, ACC_LEN, dtype=np.uint64)
    nb = (READ + 1) // 2
    pool = (rng.integers(0, 4, size=n * nb, dtype=np.uint8) | (rng.integers(0, 4, size=n * nb, dtype=np.uint8) << 4)).astype(np.uint8)
    d_pool = hip.array(pool)
    for label, nhit in (("most records on 5 accessions", 5), ("spread over 500 accessions", NACC)):
        if nhit < NACC:
            acc = np.where(rng.random(n) < 0.95, rng.integers(0, nhit, size=n), rng.integers(0, NACC, size=n)).astype(np.uint32)
        else:
            acc = rng.integers(0, NACC, size=n).astype(np.uint32)
        pos = rng.integers(0, ACC_LEN - READ, size=n).astype(np.uint32)
        recs = np.zeros(n, dtype=_hip.REC_DTYPE)
        recs["ref_new"], recs["matched"], recs["total"], recs["flag_len"] = acc, READ, READ, READ << 12
        places = np.zeros(n, dtype=_hip.PLACE_DTYPE)
        places["pos0"], places["span"] = pos, READ
        ent = np.zeros(n, dtype=_hip.BASES_DTYPE)
        ent["off"], ent["pos0"], ent["span"] = np.arange(n, dtype=np.uint64) * nb, pos, READ
        d_r, d_p, d_e = hip.array(recs.view(np.uint8)), hip.array(places.view(np.uint8)), hip.array(ent.view(np.uint8))

        def timed(make, side, after=None):
            dev = make()
            hip.sync()
            t0 = time.perf_counter()
            dev.add_ptr(d_r.ptr, side, n, 0.5)
            hip.sync()
            dt = time.perf_counter() - t0
            extra = None
            if after:
                t0 = time.perf_counter()
                res = after(dev)
                extra = (time.perf_counter() - t0, res)
            dev.free()
            return dt, extra

        def variants():
            return timed(lambda: hip.variants(lengths), (d_e.ptr, d_pool.ptr), lambda dev: dev.finish(5, 2, 50))
        variants()
        runs = [variants() for _ in range(a.reps)]
        t_cov = min(timed(lambda: hip.coverage(lengths), d_p.ptr)[0] for _ in range(a.reps + 1))
        t_dep = min(timed(lambda: hip.depth(lengths), d_p.ptr)[0] for _ in range(a.reps + 1))
        t_var, t_fin = min(r[0] for r in runs), min(r[1][0] for r in runs)
        aln, call, poly, pairs, disc, unpiled, nsites = runs[0][1][1]
        assert int(aln.sum()) == n and unpiled == 0
        say("%-30s mg_variants_add_dev %8.3f ms (%.0f M records/s, %.2f G adds/s)   mg_depth_add_dev %8.3f ms   mg_coverage_add_dev %8.3f ms"
            % (label, t_var * 1e3, n / t_var / 1e6, n * READ / t_var / 1e9, t_dep * 1e3, t_cov * 1e3))
        say("%-30s mg_variants_finish  %8.3f ms (%.1f GB of counts; %d callable, %d polymorphic sites)"
            % ("", t_fin * 1e3, NACC * ACC_LEN * 16 / 1e9, int(call.sum()), nsites))
        d_r.free()
        d_p.free()
        d_e.free()
    d_pool.free()


def tokeniser(say, hip, accs, text, a):
    idx = hip.acc_index(["Unmapped"] + accs)
    d_text = hip.array(text)

    def tokenise(**want):
        hip.sync()
        t0 = time.perf_counter()
        b = hip.sam_tokenize_dev_batch(d_text.ptr, text.size, idx, **want)
        hip.sync()
        dt = time.perf_counter() - t0
        n = b.count
        b.free()
        return dt, n
    say("tokeniser, %.1f MB of SAM text resident, %d records" % (text.size / 1e6, tokenise(based=True)[1]))
    base = None
    for name, want in (("mg_sam_tokenize_dev_ex, MG_BATCH_PLACES", {"placed": True}),
                       ("mg_sam_tokenize_dev_ex, MG_BATCH_BASES", {"based": True}),
                       ("mg_sam_tokenize_dev_ex, PLACES | BASES", {"placed": True, "based": True})):
        tokenise(**want)
        t = cp.best(lambda: tokenise(**want)[0], a.reps)
        base = t if base is None else base
        say("  %-42s %8.3f ms   (+%.3f ms)" % (name, t * 1e3, (t - base) * 1e3))
    d_text.free()
    idx.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true", help="only the end-to-end runs")
    ap.add_argument("--kernels", action="store_true", help="only the kernels")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    hip = _hip.Hip.get(0)
    rng = np.random.default_rng(20261020)
    if a.kernels:
        kernels(say, hip, rng, a)
        return
    with tempfile.TemporaryDirectory() as d:
        accs, text = cp.write_case(d, a.lines, rng)
        if not a.e2e:
            kernels(say, hip, rng, a)
            tokeniser(say, hip, accs, text, a)
        end_to_end(say, d, a.reps)


if __name__ == "__main__":
    main()
