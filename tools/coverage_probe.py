"""What --coverage costs on the device.

Kernels: mg_coverage_add_dev and the count of mg_coverage_result over --records synthetic 150-base records on 500 accessions of
4 Mb, in name order (random places) and in coordinate order (sorted by accession and place), spread over all accessions (low
depth, low contention) and piled on ten of them (depth ~40: most bits are already set, most sums go to a few bins).
Tokeniser: mg_sam_tokenize_dev against mg_sam_tokenize_dev_ex with MG_BATCH_PLACES on the same resident SAM text of --lines lines
(10 M by default, 3.6 GB: one 150-base record per line).  End to end: map_and_profile over that text as a file, with and without --coverage (--e2e alone runs at any commit: without the
flag it uses nothing this tool's other parts need).  Best of --reps; for the end-to-end runs every repeat is printed.

    python tools/coverage_probe.py --out profiles/r08/coverage_probe.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MG_PROBE_ROOT", ROOT))

from metalign_amd import _hip  # noqa: E402

NACC, ACC_LEN, READ = 500, 4_000_000, 150


def best(fn, reps):
    return min(fn() for _ in range(reps))


def _digits(arr, col, width, values):
    """values, zero-padded to `width` decimal digits, into columns col .. of every row."""
    v = values.astype(np.int64)
    for k in range(width):
        arr[:, col + width - 1 - k] = (v % 10 + 48).astype(np.uint8)
        v //= 10


def write_case(d, lines, rng):
    """A db_info file and a SAM file of `lines` alignment lines (one 150-base read each) with @SQ lines and places all over the
    accessions.  Every line has the same width (numbers zero-padded), so the text is one numpy array filled column by column."""
    accs = ["NZ_PRB%06d.1" % i for i in range(1, NACC + 1)]
    with open(os.path.join(d, "db_info.txt"), "w") as fh:
        fh.write("Accesion\tLength\tTaxID\tLineage\tTaxID_Lineage\n")
        fh.write("Unmapped\t0\tUnmapped\t|||||||Unmapped\t|||||||Unmapped\n")
        for i, a in enumerate(accs):
            ids = ["2", "10", "20", "30", "40", "50", str(1000 + i // 4), str(900000 + i // 2)]
            fh.write("%s\t%d\t%s\t%s\t%s\n" % (a, ACC_LEN, ids[-1], "|".join("n" + x for x in ids), "|".join(ids)))
    seq = "ACGT" * 37 + "AC"
    head = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (a, ACC_LEN) for a in accs)).encode()
    fields = ["read_000000000", "000", "NZ_PRB000000.1", "0000000", "60", "150M", "*", "0", "0", seq, "I" * len(seq), "NM:i:1"]
    row = np.frombuffer(("\t".join(fields) + "\n").encode(), dtype=np.uint8)
    col = np.cumsum([0] + [len(f) + 1 for f in fields])
    body = np.tile(row, (lines, 1))
    _digits(body, int(col[0]) + 5, 9, np.arange(1, lines + 1))
    _digits(body, int(col[1]), 3, np.where(rng.random(lines) < 0.5, 16, 0))
    _digits(body, int(col[2]) + 6, 6, rng.integers(1, NACC + 1, size=lines))
    _digits(body, int(col[3]), 7, rng.integers(1, ACC_LEN - READ, size=lines))
    text = np.concatenate([np.frombuffer(head, dtype=np.uint8), body.reshape(-1)])
    text.tofile(os.path.join(d, "probe.sam"))
    return accs, text


def end_to_end(say, d, reps):
    import argparse as ap
    from metalign_amd import cli, map_and_profile as mp

    def run(cov):
        args = ap.Namespace(infiles=[os.path.join(d, "probe.sam")], data="data/", db="NONE", dbinfo=os.path.join(d, "db_info.txt"),
                            input_type="sam", length_normalize=False, low_mem=False, min_abundance=10 ** -4, rank_renormalize=False,
                            output=os.path.join(d, "out.cami"), pct_id=0.5, no_quantify_unmapped=False, read_cutoff=1, sampleID="probe",
                            threads=4, verbose=False)
        if cov:
            args.coverage = os.path.join(d, "cov.tsv")
        t0 = time.perf_counter()
        mp.map_main(args)
        return time.perf_counter() - t0
    run(False)
    t = [run(False) for _ in range(reps)]
    say("map_and_profile end to end, no flag      %s ms   (median %.2f, spread %.2f)"
        % (" ".join("%.2f" % (x * 1e3) for x in t), float(np.median(t)) * 1e3, (max(t) - min(t)) * 1e3))
    if any(a.dest == "coverage" for a in cli.parser_for("map_and_profile")._actions):  # (the commit under test has the flag)
        run(True)
        t = [run(True) for _ in range(reps)]
        say("map_and_profile end to end, --coverage   %s ms   (median %.2f, spread %.2f)"
            % (" ".join("%.2f" % (x * 1e3) for x in t), float(np.median(t)) * 1e3, (max(t) - min(t)) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true", help="only the end-to-end runs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")

    hip = _hip.Hip.get(0)
    rng = np.random.default_rng(20261019)
    with tempfile.TemporaryDirectory() as d:
        accs, text = write_case(d, a.lines, rng)
        if not a.e2e:
            kernels(say, hip, rng, a)
            tokeniser(say, hip, accs, text, a)
        end_to_end(say, d, a.reps)


def kernels(say, hip, rng, a):
    n = a.records
    lengths = np.full(NACC, ACC_LEN, dtype=np.uint64)
    for label, nhit in (("spread over 500 accessions", NACC), ("piled on 10 accessions", 10)):
        acc = rng.integers(0, nhit, size=n).astype(np.uint32)
        pos = rng.integers(0, ACC_LEN - READ, size=n).astype(np.uint32)
        depth = n * READ / (nhit * ACC_LEN)
        for order in ("name order", "coordinate order"):
            if order == "coordinate order":
                o = np.lexsort((pos, acc))
                acc, pos = acc[o], pos[o]
            recs = np.zeros(n, dtype=_hip.REC_DTYPE)
            recs["ref_new"], recs["matched"], recs["total"], recs["flag_len"] = acc, READ, READ, READ << 12
            places = np.zeros(n, dtype=_hip.PLACE_DTYPE)
            places["pos0"], places["span"] = pos, READ
            d_r, d_p = hip.array(recs.view(np.uint8)), hip.array(places.view(np.uint8))

            def add():
                dev = hip.coverage(lengths)
                hip.sync()
                t0 = time.perf_counter()
                dev.add_ptr(d_r.ptr, d_p.ptr, n, 0.5)
                hip.sync()
                t1 = time.perf_counter()
                res = dev.result()
                t2 = time.perf_counter()
                dev.free()
                return t1 - t0, t2 - t1, res
            add()
            runs = [add() for _ in range(a.reps)]
            t_add, t_cnt = min(r[0] for r in runs), min(r[1] for r in runs)
            aln, bases, covered, unplaced = runs[0][2]
            assert int(aln.sum()) == n and unplaced == 0 and int(bases.sum()) == n * READ
            say("%-28s %-17s depth %5.2f  breadth %.3f   add_dev %8.3f ms (%.0f M records/s)   count + read-back %7.3f ms (%.0f MB bitmap)"
                % (label, order, depth, covered[:nhit].sum() / (nhit * ACC_LEN), t_add * 1e3, n / t_add / 1e6, t_cnt * 1e3,
                   NACC * ACC_LEN / 8e6))
            d_r.free()
            d_p.free()


def tokeniser(say, hip, accs, text, a):
    idx = hip.acc_index(["Unmapped"] + accs)
    raw = text
    d_text = hip.array(raw)

    def tokenise(placed):
        hip.sync()
        t0 = time.perf_counter()
        b = hip.sam_tokenize_dev_batch(d_text.ptr, raw.size, idx, placed=placed)
        hip.sync()
        dt = time.perf_counter() - t0
        n = b.count
        b.free()
        return dt, n
    tokenise(False), tokenise(True)
    t_plain = best(lambda: tokenise(False)[0], a.reps)
    t_placed = best(lambda: tokenise(True)[0], a.reps)
    say("tokeniser, %.1f MB of SAM text resident, %d records" % (raw.size / 1e6, tokenise(True)[1]))
    say("  mg_sam_tokenize_dev                        %8.3f ms" % (t_plain * 1e3))
    say("  mg_sam_tokenize_dev_ex, MG_BATCH_PLACES    %8.3f ms   (+%.3f ms)" % (t_placed * 1e3, (t_placed - t_plain) * 1e3))
    d_text.free()
    idx.free()


if __name__ == "__main__":
    main()
