"""What --read_assignments costs on the device.

Stage C: the commit pass with and without the verdict words (mg_profile_commit_dev / mg_profile_commit_assign_dev) over the same
--records alignment records resident in HBM (synth.make_alignment_records, 1.25 lines per read), and the map-only pass that sizes the
verdict array.  Tokeniser: mg_sam_tokenize_dev against mg_sam_tokenize_named_dev on the same resident SAM text.  Best of --reps.
The expectation to hold the numbers against: 16 B stored per read, and the names read once and written once.

    python tools/assign_probe.py --out profiles/r07/assign_probe.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metalign_amd import _hip, synth  # noqa: E402


def best(fn, reps):
    t = []
    for _ in range(reps):
        t.append(fn())
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")

    hip = _hip.Hip.get(0)
    rng = np.random.default_rng(synth.SEED + 9)
    nref, ntax = 2000, 500
    nreads = int(a.records / 1.25)
    recs = synth.make_alignment_records(rng.integers(1, nref, size=nreads), nref)
    ref2tax = rng.integers(0, ntax, size=nref).astype(np.uint32)
    d_recs, d_r2t = hip.array(recs), hip.array(ref2tax)
    d_acc = hip.empty(3 * ntax + 2, np.uint64)
    base = d_acc.ptr
    acc_args = (base, base + 8 * ntax, base + 16 * ntax, base + 24 * ntax)
    reads = int((recs["ref_new"] >> 31).sum())
    d_words = hip.empty(2 * reads, np.uint64)

    def map_only():
        s = hip.profile_begin_dev(d_recs.ptr, len(recs), False, d_r2t.ptr, nref, ntax, 0.5)
        hip.sync()
        t0 = time.perf_counter()
        n = s.ngroups
        dt = time.perf_counter() - t0
        assert n == reads
        s.free()
        return dt

    def commit(assign):
        s = hip.profile_begin_dev(d_recs.ptr, len(recs), False, d_r2t.ptr, nref, ntax, 0.5)
        if assign:
            assert s.ngroups == reads  # (the map-only pass: timed on its own above)
        hip.sync()
        t0 = time.perf_counter()
        if assign:
            s.commit_assign(True, True, 0, *acc_args, d_words.ptr)
        else:
            s.commit(True, True, 0, *acc_args, reset=True)
        hip.stage_c_join()
        hip.sync()
        dt = time.perf_counter() - t0
        s.free()
        return dt

    commit(False), commit(True)  # (warm: buffers pooled, code loaded)
    say("stage C, %d records, %d reads resident" % (len(recs), reads))
    t_map, t_plain, t_assign = best(map_only, a.reps), best(lambda: commit(False), a.reps), best(lambda: commit(True), a.reps)
    say("  map-only pass (sizes the verdict array)   %8.3f ms" % (t_map * 1e3))
    say("  commit                                     %8.3f ms" % (t_plain * 1e3))
    say("  commit + verdict words                     %8.3f ms   (+%.3f ms for %.1f MB of words: %.0f GB/s if it were the stores alone)"
        % (t_assign * 1e3, (t_assign - t_plain) * 1e3, 16 * reads / 1e6, 16 * reads / max(t_assign - t_plain, 1e-9) / 1e9))
    for x in (d_words, d_acc, d_r2t, d_recs):
        x.free()

    # the tokeniser on resident text
    accs = ["NZ_SYN%06d.1" % i for i in range(1, 400)]
    idx = hip.acc_index(["Unmapped"] + accs)
    seq = "ACGT" * 37 + "AC"
    qual = "I" * len(seq)
    pick = rng.integers(0, len(accs), size=a.lines)
    sec = rng.random(a.lines) < 0.2
    parts, r = [], 0
    for i in range(a.lines):
        if not sec[i]:
            r += 1
        parts.append("read_%09d/%d\t%d\t%s\t1000\t60\t150M\t*\t0\t0\t%s\t%s\tNM:i:1\n"
                     % (r, r % 7, 256 if sec[i] else 0, accs[pick[i]], "*" if sec[i] else seq, "*" if sec[i] else qual))
    text = np.frombuffer("".join(parts).encode(), dtype=np.uint8)
    d_text = hip.array(text)

    def tokenise(named):
        hip.sync()
        t0 = time.perf_counter()
        b = hip.sam_tokenize_dev_batch(d_text.ptr, text.size, idx, named=named)
        hip.sync()
        dt = time.perf_counter() - t0
        info = (b.count, len(b.names()[1]) - 1, len(b.names()[0])) if named else (b.count, 0, 0)
        b.free()
        return dt, info

    tokenise(False), tokenise(True)
    t_plain = best(lambda: tokenise(False)[0], a.reps)
    t_named = best(lambda: tokenise(True)[0], a.reps)
    _, (n, nnames, nbytes) = tokenise(True)
    say("tokeniser, %.1f MB of SAM text resident, %d records, %d names of %.1f MB" % (text.size / 1e6, n, nnames, nbytes / 1e6))
    say("  mg_sam_tokenize_dev                        %8.3f ms" % (t_plain * 1e3))
    say("  mg_sam_tokenize_named_dev                  %8.3f ms   (+%.3f ms)" % (t_named * 1e3, (t_named - t_plain) * 1e3))
    d_text.free()
    idx.free()


if __name__ == "__main__":
    main()
