"""What --side_reads unique costs on the device ("Side outputs from uniquely assigned reads").

mg_records_mask_unique_dev (its three launches together) into a copy and in place, beside mg_identity_add_dev on the same
--records synthetic records: reads of two records on average, seven reads in ten unique, 95 % of the records on 5 of 500
accessions (tools/identity_probe.py's contended mix).  Host clock around a synchronise, best and median of --reps, every repeat
printed; the kept count is checked against the definition (side_reads.unique_mask_of_records) first.

    python tools/sidemask_probe.py --out profiles/r11/sidemask_probe.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from metalign_amd import _hip, side_reads  # noqa: E402

NACC, NTAX, READ = 500, 100, 150


def case(n, rng):
    new = rng.random(n) < 0.5
    new[0] = True
    acc = np.where(rng.random(n) < 0.95, rng.integers(0, 5, size=n), rng.integers(0, NACC, size=n)).astype(np.uint32)
    recs = np.zeros(n, dtype=_hip.REC_DTYPE)
    recs["ref_new"] = acc | (new.astype(np.uint32) << np.uint32(31))
    recs["matched"], recs["total"], recs["flag_len"] = READ, READ, READ << 12
    edits = np.zeros(n, dtype=_hip.EDIT_DTYPE)
    edits["nm"], edits["cols"] = rng.integers(0, 7, size=n).astype(np.uint32), READ
    ref2tax = (np.arange(NACC) % NTAX).astype(np.uint32)
    nreads = int(new.sum())
    kind = rng.choice([0, 1, 1, 1, 1, 1, 1, 1, 2, 2], nreads).astype(np.uint64)
    first = np.flatnonzero(new)
    # (a unique read is counted for the taxon of one of its lines: here that of the line that opens it, or the next one)
    tax = ref2tax[acc[np.minimum(first + rng.integers(0, 2, size=nreads), n - 1)]].astype(np.uint64)
    words = np.zeros(2 * nreads, dtype=np.uint64)
    words[0::2] = kind | (tax << np.uint64(2)) * (kind == 1)
    return recs, edits, words, ref2tax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    hip = _hip.Hip.get(0)
    n = a.records
    recs, edits, words, ref2tax = case(n, np.random.default_rng(20261020))
    want = int(side_reads.unique_mask_of_records(recs, words, ref2tax).sum())
    d_r, d_e, d_w, d_t = hip.array(recs.view(np.uint8)), hip.array(edits.view(np.uint8)), hip.array(words), hip.array(ref2tax)
    d_o, d_s = hip.empty(16 * n, np.uint8), hip.array(np.zeros(2, dtype=np.uint64))

    def mask(dst):
        hip.sync()
        t0 = time.perf_counter()
        hip._chk(hip.lib.mg_records_mask_unique_dev(ctypes.c_void_p(d_r.ptr), ctypes.c_uint64(n), ctypes.c_void_p(d_w.ptr),
                                                    ctypes.c_uint64(len(words) // 2), ctypes.c_void_p(d_t.ptr), ctypes.c_uint32(NACC),
                                                    ctypes.c_void_p(dst), ctypes.c_void_p(d_s.ptr)))
        hip.sync()
        return time.perf_counter() - t0

    def ident(src):
        dev = hip.identity(NACC)
        hip.sync()
        t0 = time.perf_counter()
        dev.add_ptr(src, d_e.ptr, n, 0.5)
        hip.sync()
        dt = time.perf_counter() - t0
        dev.free()
        return dt

    mask(d_o.ptr)
    kept, outside = (int(x) for x in d_s.download())
    assert (kept, outside) == (want, 0), (kept, outside, want)
    say("%d records, %d reads, %d kept (%.1f %%): equal to the definition" % (n, len(words) // 2, kept, 100.0 * kept / n))
    ident(d_r.ptr)
    rows = [("mg_records_mask_unique_dev into a copy", lambda: mask(d_o.ptr)), ("mg_identity_add_dev, every record", lambda: ident(d_r.ptr)),
            ("mg_identity_add_dev, the masked copy", lambda: ident(d_o.ptr)), ("mg_records_mask_unique_dev in place", lambda: mask(d_r.ptr))]
    for label, fn in rows:  # (in place last: it changes the records)
        t = [fn() * 1e3 for _ in range(a.reps)]
        say("%-42s best %7.3f ms  median %7.3f ms   (%s)" % (label, min(t), float(np.median(t)), " ".join("%.3f" % x for x in t)))
    for d in (d_r, d_e, d_w, d_t, d_o, d_s):
        d.free()


if __name__ == "__main__":
    main()
