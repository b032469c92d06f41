"""The iterated multimapped-read reassignment (--multimap_iterations) on the device against the one-step kernel and the host routine:
reads -> classes, the time to build the classes, the time per iteration, k_resolve_multimapped's one step over the same CSR, and
mg_multimapped_shares_iter's time per iteration.  Two CSRs: one whose reads collapse into few classes (G genomes, lists of 2-8), one in
which nearly every read is a class of its own (lists of 3 out of 2^20 genomes).
Usage: python tools/multimap_iter_probe.py [R reads] [G genomes] [N iterations] [--no-host]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from metalign_amd import _hip  # noqa: E402
from metalign_amd._hip import Hip  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
R = int(argv[0]) if len(argv) > 0 else 10_000_000
G = int(argv[1]) if len(argv) > 1 else 37
N = int(argv[2]) if len(argv) > 2 else 12
HOST = "--no-host" not in sys.argv


def records(rng, nreads, ntax, lo, hi):
    """Single-end reads of lo..hi-1 retained lines each (a multimapped list in file order); a dummy read of two lines first (the read
    behind the file's first boundary loses a line) and one last (the last read is never processed)."""
    lens = rng.integers(lo, hi, size=nreads).astype(np.int64)
    first = np.full(nreads + 1, 2, dtype=np.int64)
    first[1:] += np.cumsum(lens)
    n = int(first[-1]) + 1
    recs = np.zeros(n, dtype=_hip.REC_DTYPE)
    recs["total"] = 100
    recs["matched"] = 100
    recs["ref_new"] = rng.integers(0, ntax, size=n).astype(np.uint32)
    recs["ref_new"][first] |= np.uint32(_hip.NEW_BIT)
    recs["ref_new"][0] |= np.uint32(_hip.NEW_BIT)
    recs["ref_new"][1] = recs["ref_new"][0] & np.uint32(_hip.NEW_BIT - 1)
    recs["flag_len"][first[:-1]] = rng.integers(100, 151, size=nreads).astype(np.uint32) << np.uint32(_hip.LEN_SHIFT)
    return recs


def probe(hip, tag, ntax, lo, hi):
    rng = np.random.default_rng(11)
    recs = records(rng, R, ntax, lo, hi)
    rd = hip.profile_assign_resident(recs, np.arange(ntax, dtype=np.uint32), ntax, 0.5)
    res = rd["resident"]
    w0 = rng.integers(1000, 10 ** 6, size=ntax).astype(np.float64)
    w0[rng.random(ntax) < 0.1] = np.nan
    hip.prof_enable(True)
    res.resolve_multimapped(w0)  # (warm: buffers, code objects)
    res.iterate_multimapped(w0, None, 2, 0.0)
    hip.prof_reset()
    one_step = res.resolve_multimapped(w0)
    _, t_step = hip.prof_get("resolve_multimapped")
    hip.prof_reset()
    t0 = time.perf_counter()
    extra1, _, _, ncls = res.iterate_multimapped(w0, None, 1, 0.0)
    t_call1 = time.perf_counter() - t0
    _, t_build = hip.prof_get("mm_classes")
    _, t_it1 = hip.prof_get("mm_iterate")
    hip.prof_reset()
    t0 = time.perf_counter()
    extra_n, ran, change, _ = res.iterate_multimapped(w0, None, N, 0.0)
    t_calln = time.perf_counter() - t0
    _, t_itn = hip.prof_get("mm_iterate")
    hip.prof_enable(False)
    ok = one_step != 0
    print("%s: %d multimapped reads, %d entries, %d taxa -> %d classes" % (tag, rd["mm_nreads"], rd["mm_nentries"], ntax, ncls))
    print("  k_resolve_multimapped, one step            %9.3f ms" % t_step)
    print("  classes built (kernels, sort, scans)       %9.3f ms   (whole call with 1 iteration %.1f ms, with %d: %.1f ms)"
          % (t_build, 1e3 * t_call1, N, 1e3 * t_calln))
    print("  one iteration over classes                 %9.3f ms   (%d iterations %.3f ms; the first alone %.3f ms)"
          % (t_itn / ran, ran, t_itn, t_it1))
    print("  one iteration against the one step: largest relative difference %.2e; last change after %d iterations %.3g"
          % (float(np.max(np.abs(extra1[ok] - one_step[ok]) / one_step[ok])), ran, change))
    if HOST:
        off, tax, hl, _ = res.shard.multimapped()
        t0 = time.perf_counter()
        _hip.multimapped_shares_iter(off, tax, hl, w0, None, 1, 0.0)
        t1 = time.perf_counter()
        got = _hip.multimapped_shares_iter(off, tax, hl, w0, None, 4, 0.0)
        t2 = time.perf_counter()
        dev4 = res.iterate_multimapped(w0, None, 4, 0.0)[0]
        ok = got[0] != 0
        print("  mg_multimapped_shares_iter, per iteration  %9.3f ms   (device against host after 4: %.2e relative)"
              % (1e3 * ((t2 - t1) - (t1 - t0)) / 3, float(np.max(np.abs(dev4[ok] - got[0][ok]) / got[0][ok]))))
    res.free()


hip = Hip.get(0)
probe(hip, "collapsing", G, 2, 9)
probe(hip, "not collapsing", 1 << 20, 3, 4)
