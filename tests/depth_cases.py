"""Shared by the depth tests (CPU and -m gpu): seeded intervals over accessions whose lengths sit on the statistics' edges, a
per-base brute force, and the case file tests/host_depth_check.cpp reads."""
import random
import struct

import numpy as np

from metalign_amd import depth as dp

# the trimmed mean's t = L * 5 // 100 steps at 20 and 40; odd and even lengths take different median ranks
EDGE_LENGTHS = [1, 19, 20, 21, 39, 40, 41, 0, 2, 1023, 1024, 1025]


def random_case(seed, max_len=5000, nplaced=400):
    """-> (lengths {accession: L}, placed [(accession, pos0, span)]): the edge lengths, random ones, one accession whose positions
    all share one depth, one where the clamp works (5000 identical intervals) and unplaced intervals."""
    rng = random.Random(seed)
    lengths = {"e%d" % i: n for i, n in enumerate(EDGE_LENGTHS)}
    lengths.update({"r%d" % i: rng.randrange(1, max_len + 1) for i in range(4)})
    lengths["flat"] = rng.randrange(50, 300)
    lengths["deep"] = rng.randrange(30, 90)
    placed = []
    accs = list(lengths)
    for _ in range(rng.randrange(1, nplaced)):
        acc = rng.choice(accs[:-2])
        n = lengths[acc]
        placed.append((acc, rng.randrange(0, n + 40), rng.choice([0, 1, 2, 31, 32, 33, 64, rng.randrange(1, 700)])))
    placed += [("r0", 10, 5), ("r0", 15, 5), ("r0", 11, 2), ("r0", 10, 5)]  # touching, nested, duplicate
    placed += [("flat", 0, lengths["flat"] + 7)] * 3                          # every position at depth 3: H in one bin
    placed += [("deep", 5, 20)] * 5000 + [("deep", 0, 8)]                     # depth 5000 and 5001: clamped
    rng.shuffle(placed)
    return lengths, placed


def brute(placed, lengths, window=0):
    """The same as depth.accumulate from a per-base array per accession."""
    arrays, counts, unplaced = {}, {}, 0
    for acc, pos0, span in placed:
        n = lengths[acc]
        if span == 0 or pos0 >= n:
            unplaced += 1
            continue
        a = arrays.setdefault(acc, np.zeros(n, dtype=np.int64))
        a[pos0:min(pos0 + span, n)] += 1
        counts[acc] = counts.get(acc, 0) + 1
    per, windows = {}, {}
    for acc, a in arrays.items():
        c = np.minimum(a, dp.CAP)
        vals, cnt = np.unique(c, return_counts=True)
        per[acc] = [counts[acc], {int(v): int(k) for v, k in zip(vals, cnt)}]
        if window:
            windows[acc] = [(j, int(a[j * window:(j + 1) * window].sum()), int(np.count_nonzero(a[j * window:(j + 1) * window])))
                            for j in range((len(a) + window - 1) // window) if a[j * window:(j + 1) * window].sum() > 0]
    return per, unplaced, windows, arrays


def case_blob(lengths, placed, window):
    """The case file of host_depth_check.cpp: u32 W, u32 nacc, u64 lengths[], u32 n, then (u32 row, u32 pos0, u32 span) each."""
    accs = list(lengths)
    row = {a: i for i, a in enumerate(accs)}
    blob = struct.pack("<II", window, len(accs)) + b"".join(struct.pack("<Q", lengths[a]) for a in accs)
    blob += struct.pack("<I", len(placed)) + b"".join(struct.pack("<III", row[a], p, s) for a, p, s in placed)
    return blob, accs


def parse_check_output(text, accs):
    """host_depth_check's lines -> (per, unplaced, windows) as depth.accumulate gives them."""
    per, windows, unplaced = {}, {}, None
    for ln in text.splitlines():
        f = ln.split()
        if f[0] == "U":
            unplaced = int(f[1])
        elif f[0] == "A":
            per[accs[int(f[1])]] = [int(f[2]), {}]
        elif f[0] == "H":
            per[accs[int(f[1])]][1][int(f[2])] = int(f[3])
        elif f[0] == "W":
            windows.setdefault(accs[int(f[1])], []).append((int(f[2]), int(f[3]), int(f[4])))
        else:
            raise AssertionError(ln)
    return per, unplaced, windows
