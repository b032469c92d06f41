"""What --depth / --depth_windows cost on the device (per-base depth), with --coverage on the same records as yardstick.

--records records of 150 bases over --bases reference bases in accessions of 4 Mb, placed as synth.make_reads places its reads:
--present accessions are hit, under a log-normal(0, 1) abundance vector, at uniform positions, in name order.  Every kernel family
of mg_depth.hip is timed by the library's own device events (ProfScope: depth_add, depth_tile_sums, depth_scan_tiles, depth_hist,
depth_windows), for --window 0 and --window W; mg_coverage_add_dev + mg_coverage_result (cov_add, cov_count) run on the same device
arrays in the same process, alternating with the depth runs.  Rates are 4 B per slot of the WHOLE array over the
pass's time: both passes skip the tiles in which no hit accession owns a slot, so with few accessions hit they read less than that.

    python tools/depth_probe.py --out depth_probe.txt                  # 50 of 250 accessions hit
    python tools/depth_probe.py --present 250 --out depth_probe_all.txt  # every accession hit
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MG_PROBE_ROOT", ROOT))

from metalign_amd import _hip  # noqa: E402

ACC_LEN, READ = 4_000_000, 150
DEPTH_KERNELS = ("depth_add", "depth_tile_sums", "depth_scan_tiles", "depth_hist", "depth_windows")
COV_KERNELS = ("cov_add", "cov_count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--present", type=int, default=50)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")

    hip = _hip.Hip.get(0)
    rng = np.random.default_rng(0x4D37A + 7)
    nacc, n = max(a.bases // ACC_LEN, 1), a.records
    lengths = np.full(nacc, ACC_LEN, dtype=np.uint64)
    present = rng.choice(nacc, size=min(a.present, nacc), replace=False)
    w = rng.lognormal(0.0, 1.0, size=len(present))
    recs = np.zeros(n, dtype=_hip.REC_DTYPE)
    recs["ref_new"] = present[rng.choice(len(present), size=n, p=w / w.sum())].astype(np.uint32)
    recs["matched"], recs["total"], recs["flag_len"] = READ, READ, READ << 12
    places = np.zeros(n, dtype=_hip.PLACE_DTYPE)
    places["pos0"], places["span"] = rng.integers(0, ACC_LEN - READ, size=n).astype(np.uint32), READ
    d_r, d_p = hip.array(recs.view(np.uint8)), hip.array(places.view(np.uint8))
    slots = int(lengths.sum()) + nacc
    say("%d records of %d bases on %d of %d accessions of %d bases (%.0f MB of slots, %.0f MB of bitmap); mean depth of a hit accession %.1f"
        % (n, READ, len(present), nacc, ACC_LEN, slots * 4 / 1e6, int(lengths.sum()) / 8e6, n * READ / (len(present) * ACC_LEN)))

    def timed(kernels, fn):
        hip.prof_reset()
        hip.sync()
        t0 = time.perf_counter()
        res = fn()
        hip.sync()
        wall = time.perf_counter() - t0
        return wall, {k: hip.prof_get(k)[1] for k in kernels}, res

    def depth_run(window):
        t0 = time.perf_counter()
        dev = hip.depth(lengths, window)
        hip.sync()
        t_create = time.perf_counter() - t0
        try:
            t_add, k_add, _ = timed(DEPTH_KERNELS, lambda: dev.add_ptr(d_r.ptr, d_p.ptr, n, 0.5))
            t_fin, k_fin, res = timed(DEPTH_KERNELS, dev.finish)
            t_fetch, _, _ = timed((), lambda: (dev.fetch_rows(), dev.fetch_windows()))
        finally:
            dev.free()
        k_fin["depth_add"] = k_add["depth_add"]
        assert int(res[0].sum()) == n and res[1] == 0 and res[2] == len(present)
        return dict(create=t_create * 1e3, add=t_add * 1e3, finish=t_fin * 1e3, fetch=t_fetch * 1e3, nwin=res[3], **k_fin)

    def cov_run():
        t0 = time.perf_counter()
        dev = hip.coverage(lengths)
        hip.sync()
        t_create = time.perf_counter() - t0
        try:
            t_add, k_add, _ = timed(COV_KERNELS, lambda: dev.add_ptr(d_r.ptr, d_p.ptr, n, 0.5))
            t_res, k_res, res = timed(COV_KERNELS, dev.result)
        finally:
            dev.free()
        assert int(res[0].sum()) == n and res[3] == 0
        return dict(create=t_create * 1e3, add=t_add * 1e3, result=t_res * 1e3, cov_add=k_add["cov_add"], cov_count=k_res["cov_count"])

    hip.prof_enable(True)
    try:
        cov_run(), depth_run(0), depth_run(a.window)  # warm-up of every shape
        runs = {"cov": [], 0: [], a.window: []}
        for _ in range(a.reps):  # alternating
            runs["cov"].append(cov_run())
            runs[0].append(depth_run(0))
            runs[a.window].append(depth_run(a.window))
    finally:
        hip.prof_enable(False)
        d_r.free()
        d_p.free()

    def row(label, rs, key, nbytes=0):
        v = sorted(r[key] for r in rs)
        rate = "   %6.2f TB/s of %.2f GB" % (nbytes / (v[len(v) // 2] * 1e-3) / 1e12, nbytes / 1e9) if nbytes and v[len(v) // 2] > 0 else ""
        say("  %-44s median %9.3f ms   min %9.3f   max %9.3f%s" % (label, v[len(v) // 2], v[0], v[-1], rate))

    say("--coverage (yardstick)")
    row("k_cov_add (device events)", runs["cov"], "cov_add")
    row("k_cov_count (device events)", runs["cov"], "cov_count")
    row("create: hipMalloc + memset (host clock)", runs["cov"], "create")
    row("add_dev + sync (host clock)", runs["cov"], "add")
    row("result (host clock)", runs["cov"], "result")
    for window in (0, a.window):
        rs = runs[window]
        say("--depth, window %d (%d windows kept)" % (window, rs[0]["nwin"]))
        row("k_depth_add (device events)", rs, "depth_add")
        row("k_depth_tile_sums (device events)", rs, "depth_tile_sums", 4 * slots)
        row("k_depth_scan_tiles (device events)", rs, "depth_scan_tiles")
        row("k_depth_hist, windows fused (device events)", rs, "depth_hist", 4 * slots)
        row("k_depth_win_compact x2 (device events)", rs, "depth_windows")
        row("create: hipMalloc + memset (host clock)", rs, "create")
        row("add_dev + sync (host clock)", rs, "add")
        row("finish (host clock)", rs, "finish")
        row("both fetches (host clock)", rs, "fetch")


if __name__ == "__main__":
    main()
