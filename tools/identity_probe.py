"""What --identity costs on the device.

Kernels: mg_identity_add_dev against mg_coverage_add_dev on the same --records synthetic 150-base records, in two mixes: most
records on a few accessions with identities in a few dozen bins near 1000 (a real sample: the worst case for atomics), and records
spread evenly over 500 accessions and all bins.
Tokeniser: mg_sam_tokenize_dev against mg_sam_tokenize_dev_ex with MG_BATCH_PLACES, with MG_BATCH_EDITS and with both, on the same
resident SAM text of --lines lines (tools/coverage_probe.py's file: 10 M lines by default, 3.6 GB, NM:i: the twelfth field), and with
NM:i: behind five other tags.
End to end: map_and_profile over that text as a file, with and without --identity (--e2e alone runs at any commit: without the flag
it uses nothing this tool's other parts need; MG_PROBE_ROOT names the package to import; --all_flags adds a run with --coverage, --depth
and --identity together; a flag the commit's parser does not have is left out).  Best of --reps for the kernels and the
tokeniser; for the end-to-end runs every repeat is printed.

    python tools/identity_probe.py --out profiles/r10/identity_probe.txt
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


def end_to_end(say, d, reps, all_flags=False):
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
    # (the parser says which flags the commit under test has)
    known = {a.dest for a in cli.parser_for("map_and_profile")._actions}
    configs = [("no flag", ()), ("--identity", ("identity",))]
    if all_flags:
        configs.append(("--coverage --depth --identity", ("coverage", "depth", "identity")))
    for label, flags in configs:
        if not set(flags) <= known:
            continue
        run(flags)
        t = [run(flags) for _ in range(reps)]
        say("map_and_profile end to end, %-12s %s ms   (median %.2f, spread %.2f)"
            % (label, " ".join("%.2f" % (x * 1e3) for x in t), float(np.median(t)) * 1e3, (max(t) - min(t)) * 1e3))


def kernels(say, hip, rng, a):
    n = a.records
    lengths = np.full(NACC, ACC_LEN, dtype=np.uint64)
    for label, nhit in (("most records on 5 accessions, bins near 1000", 5), ("spread over 500 accessions and all bins", NACC)):
        if nhit < NACC:  # 95 % of the records on nhit accessions, 0 to 6 edits; the rest anywhere, up to 40
            acc = np.where(rng.random(n) < 0.95, rng.integers(0, nhit, size=n), rng.integers(0, NACC, size=n)).astype(np.uint32)
            nm = np.where(rng.random(n) < 0.95, rng.integers(0, 7, size=n), rng.integers(0, 41, size=n)).astype(np.uint32)
        else:
            acc = rng.integers(0, NACC, size=n).astype(np.uint32)
            nm = rng.integers(0, READ + 1, size=n).astype(np.uint32)
        recs = np.zeros(n, dtype=_hip.REC_DTYPE)
        recs["ref_new"], recs["matched"], recs["total"], recs["flag_len"] = acc, READ, READ, READ << 12
        edits = np.zeros(n, dtype=_hip.EDIT_DTYPE)
        edits["nm"], edits["cols"] = nm, READ
        places = np.zeros(n, dtype=_hip.PLACE_DTYPE)
        places["pos0"], places["span"] = rng.integers(0, ACC_LEN - READ, size=n).astype(np.uint32), READ
        d_r, d_e, d_p = hip.array(recs.view(np.uint8)), hip.array(edits.view(np.uint8)), hip.array(places.view(np.uint8))

        def ident():
            dev = hip.identity(NACC)
            hip.sync()
            t0 = time.perf_counter()
            dev.add_ptr(d_r.ptr, d_e.ptr, n, 0.5)
            hip.sync()
            dt = time.perf_counter() - t0
            res = dev.sums()
            dev.free()
            return dt, res

        def cover():
            dev = hip.coverage(lengths)
            hip.sync()
            t0 = time.perf_counter()
            dev.add_ptr(d_r.ptr, d_p.ptr, n, 0.5)
            hip.sync()
            dt = time.perf_counter() - t0
            dev.free()
            return dt
        ident(), cover()
        runs = [ident() for _ in range(a.reps)]
        t_cov = min(cover() for _ in range(a.reps))
        t_id = min(r[0] for r in runs)
        aln, cols, eds, unscored = runs[0][1]
        assert int(aln.sum()) == n and unscored == 0 and int(cols.sum()) == n * READ and int(eds.sum()) == int(nm.sum())
        say("%-46s mg_identity_add_dev %8.3f ms (%.0f M records/s)   mg_coverage_add_dev %8.3f ms   identity %.4f"
            % (label, t_id * 1e3, n / t_id / 1e6, t_cov * 1e3, 1 - eds.sum() / cols.sum()))
        d_r.free()
        d_e.free()
        d_p.free()


def tokeniser(say, hip, accs, text, a):
    idx = hip.acc_index(["Unmapped"] + accs)

    def measure(raw, label):
        d_text = hip.array(raw)

        def tokenise(**want):
            hip.sync()
            t0 = time.perf_counter()
            b = hip.sam_tokenize_dev_batch(d_text.ptr, raw.size, idx, **want)
            hip.sync()
            dt = time.perf_counter() - t0
            n = b.count
            b.free()
            return dt, n
        say("tokeniser, %.1f MB of SAM text resident (%s), %d records" % (raw.size / 1e6, label, tokenise(edited=True)[1]))
        base = None
        for name, want in (("mg_sam_tokenize_dev", {}), ("mg_sam_tokenize_dev_ex, MG_BATCH_PLACES", {"placed": True}),
                           ("mg_sam_tokenize_dev_ex, MG_BATCH_EDITS", {"edited": True}),
                           ("mg_sam_tokenize_dev_ex, PLACES | EDITS", {"placed": True, "edited": True})):
            tokenise(**want)
            t = cp.best(lambda: tokenise(**want)[0], a.reps)
            base = t if base is None else base
            say("  %-42s %8.3f ms   (+%.3f ms)" % (name, t * 1e3, (t - base) * 1e3))
        d_text.free()
    measure(text, "NM:i: the twelfth field")
    # the same lines with five tags in front of NM:i: (every line keeps one width)
    old, new = b"\tNM:i:1\n", b"\tAS:i:290\tms:i:290\tnn:i:0\ttp:A:P\tcm:i:25\tNM:i:1\n"
    head = int(np.flatnonzero(text[:1 << 22] == 10)[NACC]) + 1  # (the @HD line and NACC @SQ lines)
    body = text[head:].reshape(-1, cp_row_width(text, head))
    wide = np.empty((body.shape[0], body.shape[1] - len(old) + len(new)), dtype=np.uint8)
    wide[:, :body.shape[1] - len(old)] = body[:, :body.shape[1] - len(old)]
    wide[:, body.shape[1] - len(old):] = np.frombuffer(new, dtype=np.uint8)
    measure(np.concatenate([text[:head], wide.reshape(-1)]), "NM:i: behind five tags")
    idx.free()


def cp_row_width(text, head):
    return int(np.flatnonzero(text[head:head + (1 << 16)] == 10)[0]) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true", help="only the end-to-end runs")
    ap.add_argument("--kernels", action="store_true", help="only the kernels")
    ap.add_argument("--all_flags", action="store_true", help="end to end also with --coverage --depth --identity together")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    hip = _hip.Hip.get(0)
    rng = np.random.default_rng(20261019)
    if a.kernels:
        kernels(say, hip, rng, a)
        return
    with tempfile.TemporaryDirectory() as d:
        accs, text = cp.write_case(d, a.lines, rng)
        if not a.e2e:
            kernels(say, hip, rng, a)
            tokeniser(say, hip, accs, text, a)
        end_to_end(say, d, a.reps, a.all_flags)


if __name__ == "__main__":
    main()
