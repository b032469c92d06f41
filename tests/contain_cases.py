"""Read sketches and hash-major tables whose ENTRIES lie where stage B's kernels change path (mg_contain.hip), and what the
definition makes of them.  Shared by test_contain_cases_host.py (every family reaches what it claims; the definition is the
oracle's) and test_gpu_contain_geometry.py (the kernels).  numpy only: no GPU, no oracle.

Three things live here and they are kept apart:

  * THE DEFINITION: expected() for a sketch against a table, matched_by_hash() / matched_by_identity() / refpipe_expected() for
    the reference pipeline's table.  Plain numpy over the project's rules; this is what the kernels are held to.
  * A MODEL OF THE GEOMETRY: plan_index(), geometry(), copies(), count_share() follow plan_index, the top of k_contain_pairs,
    containment_launch and refpipe_count_launch.  The model is no reference for answers: it exists so that a case can PROVE it
    reaches the edge it was built for (run length 2047 against 2048, the tile whose last pair sits in slot il / 256 = 5, ...).
    The constants it copies are read back from the source text by test_contain_cases_host.py.
  * THE CASE FAMILIES: functions that return lists of named cases.

A Case's sketch is given twice: `feed_*`, `s`, `set_bound` say how the handle is made (sketch_from_pairs_dev, then
Sketch.set_bound), and `q_*`, `truncated`, `bound` say what the library makes of that by its own rules — the smallest `s` of the
fed hashes, truncated when something was cut, complete up to its last hash unless set_bound said otherwise (effective_sketch;
test_contain_cases_host.py holds the two together).  Counts stay within 0 .. 3: the library's counters saturate at 3.

Hashes are 0 .. 2^64 - 2: 2^64 - 1 is the reserved value that no sketch and no table holds.

Out of scope: the `lb < 27` cap of plan_index takes a sketch of a billion entries.
"""
import functools
from collections import namedtuple

import numpy as np

U64 = np.uint64
INF = (1 << 64) - 1           # "no completeness bound" (also the reserved hash)
TOP = (1 << 64) - 2           # the largest hash
NONE = 0xFFFFFFFF             # pb: the other strand's prefix is not in D_k

# ---- what the model copies from mg_contain.hip (held to the source text by test_contain_cases_host.py)
KCT = 256                     # kCT: threads per workgroup
KCTILE = 8 * KCT              # kCTile: pairs per tile
KCCAP = 2048                  # kCCap: sketch entries staged in LDS; a run is staged when len < kCCap
PER_BUCKET = 8                # plan_index: about eight sketch entries per bucket
LB_MAX = 27                   # plan_index: at most 2^27 buckets
COPIES_MAX = 64               # containment_launch: counter copies double while copies < 64 and copies * 2 * G <= 65536
COPIES_BUDGET = 65536

Case = namedtuple("Case", "name feed_hashes feed_counts s set_bound q_hashes q_counts truncated bound pair_hash pair_gen gsize ngenomes")
Tile = namedtuple("Tile", "t0 t1 h_first h_last lo hi run_len staged pow2 slot")
Geometry = namedtuple("Geometry", "shift buckets tiles")


def u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


# ================================================================ the definition ================================================
def expected(q_hashes, q_counts, truncated, bound, ci, pair_hash, pair_gen, gsize):
    """-> (hits u32[G], sizes u32[G]).  A pair (h, g) takes part iff the sketch is not truncated or h <= bound; it hits iff h is in
    the sketch with count >= ci; sizes[g] = gsize[g] when the sketch is not truncated, else the pairs of g that take part.  Per
    pair: a pair listed twice counts twice."""
    q_hashes, q_counts = np.asarray(q_hashes, dtype=np.uint64), np.asarray(q_counts, dtype=np.uint32)
    pair_hash, pair_gen = np.asarray(pair_hash, dtype=np.uint64), np.asarray(pair_gen, dtype=np.int64)
    g = len(gsize)
    part = pair_hash <= U64(bound) if truncated else np.ones(len(pair_hash), dtype=bool)
    hit = np.zeros(len(pair_hash), dtype=bool)
    if len(q_hashes) and len(pair_hash):
        at = np.minimum(np.searchsorted(q_hashes, pair_hash, side="left"), len(q_hashes) - 1)
        hit = (q_hashes[at] == pair_hash) & (q_counts[at] >= ci)
    hits = np.bincount(pair_gen[part & hit], minlength=g).astype(np.uint32)
    sizes = np.bincount(pair_gen[part], minlength=g).astype(np.uint32) if truncated else np.asarray(gsize, dtype=np.uint32).copy()
    return hits, sizes


def effective_sketch(feed_hashes, feed_counts, s, set_bound):
    """What the library makes of (sketch_from_pairs_dev(feed, s), then set_bound): -> (q_hashes, q_counts, truncated, bound)."""
    order = np.argsort(feed_hashes, kind="stable")
    h, c = np.asarray(feed_hashes, dtype=np.uint64)[order], np.asarray(feed_counts, dtype=np.uint32)[order]
    assert len(np.unique(h)) == len(h)  # (the cases feed every hash once: no sums to state)
    truncated = bool(s > 0 and len(h) > s)
    if truncated:
        h, c = h[:s], c[:s]
    bound = int(h[-1]) if (truncated and len(h)) else INF
    if set_bound is not None:
        truncated = bool(set_bound[0])
        bound = int(set_bound[1]) if truncated else INF
    return h, c, truncated, bound


def want(case, ci):
    return expected(case.q_hashes, case.q_counts, case.truncated, case.bound, ci, case.pair_hash, case.pair_gen, case.gsize)


def genome_major(case):
    """The table as upload_table and the oracle take it: (hashes, offsets), hash-major -> genome-major by a stable sort on genome."""
    order = np.argsort(case.pair_gen, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(case.pair_gen.astype(np.int64), minlength=case.ngenomes))]).astype(np.uint64)
    return case.pair_hash[order], offsets


# ---- the reference pipeline's table
def matched_by_hash(q_hashes, q_counts, ci, pair_hash):
    """bool[npairs]: the pair's hash is in the sketch with count >= ci."""
    one = np.ones(len(pair_hash), dtype=np.uint32)
    return expected(q_hashes, q_counts, False, INF, ci, pair_hash, np.arange(len(pair_hash)), one)[0].astype(bool)


def matched_by_identity(counts, head, ci, cs):
    """bool[npairs]: pair i is matched iff min(counts[head[i]], cs or inf) >= ci."""
    c = np.asarray(counts, dtype=np.uint64)[np.asarray(head, dtype=np.int64)]
    if cs:
        c = np.minimum(c, U64(cs))
    return c >= U64(ci)


def marks_of(matched, t):
    """bool[nprefix]: the set of pa[i], pb[i] (each != 0xffffffff) over the matched pairs."""
    m = np.zeros(int(t["nprefix"]), dtype=bool)
    for col in (t["pa"], t["pb"]):
        p = np.asarray(col)[matched]
        m[p[p != NONE].astype(np.int64)] = True
    return m


def mark_words(marked):
    """The bitmap the device keeps: bit p & 31 of word p >> 5."""
    bits = np.zeros((len(marked) + 31) // 32 * 32, dtype=np.uint8)
    bits[: len(marked)] = marked
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32) if len(bits) else np.zeros(0, np.uint32)


def count_share(ncount, rank, world):
    """The run [lo, hi) of a count list that rank `rank` of `world` streams (model of refpipe_count_launch; the runs tile the list)."""
    lo = ncount // world * rank + (ncount % world) * rank // world
    hi = ncount if rank + 1 == world else ncount // world * (rank + 1) + (ncount % world) * (rank + 1) // world
    return lo, hi


def count_hits(marked, t, ngenomes, rank=0, world=1):
    """hits_k[g] = entries (cid, cgen = g) of (this rank's run of) the count list whose cid is marked."""
    lo, hi = count_share(len(t["cid"]), rank, world)
    cid, cgen = np.asarray(t["cid"][lo:hi]).astype(np.int64), np.asarray(t["cgen"][lo:hi]).astype(np.int64)
    return np.bincount(cgen[marked[cid]], minlength=ngenomes).astype(np.uint32)


def refpipe_expected(rc, matched, rank=0, world=1):
    """-> (hits u32[K][G], sizes u32[K][G]), k ascending: the smaller k from the marks, the largest k the plain definition."""
    hits = [count_hits(marks_of(matched, t), t, rc.ngenomes, rank, world) for t in rc.small]
    sizes = [np.asarray(t["gsize"], dtype=np.uint32) for t in rc.small]
    hits.append(np.bincount(rc.pair_gen[matched].astype(np.int64), minlength=rc.ngenomes).astype(np.uint32))
    sizes.append(np.asarray(rc.gsize, dtype=np.uint32))
    return np.array(hits, dtype=np.uint32).reshape(len(rc.ks), rc.ngenomes), np.array(sizes, dtype=np.uint32).reshape(len(rc.ks), rc.ngenomes)


# ================================================================ the model =====================================================
def plan_index(q_hashes):
    """(shift, buckets) as plan_index sizes the bucket index of a sketch; None for an empty one."""
    n = len(q_hashes)
    if n == 0:
        return None
    bits = max(int(q_hashes[-1]).bit_length(), 1)
    lb = 0
    while (1 << lb) < (n + PER_BUCKET - 1) // PER_BUCKET and lb < LB_MAX:
        lb += 1
    lb = min(max(lb, 1), bits)
    return bits - lb, 1 << lb


def index_stores(q_hashes, shift):
    """How many buckets each thread i of k_build_index fills (i = 0 .. n): (bucket(q[i-1]), bucket(q[i])], one more past the end."""
    b = (np.asarray(q_hashes, dtype=np.uint64) >> U64(shift)).astype(np.int64)
    return np.concatenate([[b[0] + 1], np.diff(b), [1]])


def npairs_taking_part(case):
    """The cut of a truncated sketch (k_upper_bound_one): pairs with hash <= bound."""
    return int(np.searchsorted(case.pair_hash, U64(case.bound), side="right")) if case.truncated else len(case.pair_hash)


def geometry(q_hashes, pair_hash, npairs=None):
    """The index's shape and, per tile, what the top of k_contain_pairs computes: first and last pair, the run [lo, hi) of the
    sketch (idx[b] = first position whose hash >= b << shift), whether it is staged, the padded length, and slot = il / 256, the
    register the last pair's hash is picked from."""
    q = np.asarray(q_hashes, dtype=np.uint64)
    n = len(q)
    npairs = len(pair_hash) if npairs is None else npairs
    plan = plan_index(q)
    shift, buckets = plan if plan else (0, 0)
    qb = q >> U64(shift)
    tiles = []
    for t0 in range(0, npairs, KCTILE):
        t1 = min(t0 + KCTILE, npairs)
        h_first, h_last = int(pair_hash[t0]), int(pair_hash[t1 - 1])
        lo = hi = 0
        if n > 0 and h_first <= int(q[-1]):
            top = min(h_last, int(q[-1]))
            lo = int(np.searchsorted(qb, U64(h_first >> shift), side="left"))
            hi = int(np.searchsorted(qb, U64((top >> shift) + 1), side="left"))
        run = hi - lo
        pow2 = 1
        while pow2 <= run:
            pow2 <<= 1
        tiles.append(Tile(t0, t1, h_first, h_last, lo, hi, run, run < KCCAP, pow2, (t1 - 1 - t0) // KCT))
    return Geometry(shift, buckets, tiles)


def case_geometry(case):
    return geometry(case.q_hashes, case.pair_hash, npairs_taking_part(case))


def copies(ngenomes):
    """Replicated counter copies of a call whose largest table has `ngenomes` genomes (containment_launch)."""
    c = 1
    while c < COPIES_MAX and c * 2 * ngenomes <= COPIES_BUDGET:
        c *= 2
    return c


# ================================================================ building blocks ===============================================
def _case(name, q_hashes, q_counts, pair_hash, pair_gen, ngenomes, extra=(), set_bound=None):
    """extra: hashes above the sketch, fed with it and cut off by s = len(q): a truncated sketch, complete up to its last hash."""
    q_hashes, q_counts = np.asarray(q_hashes, dtype=np.uint64), np.asarray(q_counts, dtype=np.uint32)
    extra = np.asarray(extra, dtype=np.uint64)
    assert len(extra) == 0 or (len(q_hashes) and int(extra.min()) > int(q_hashes[-1]))
    feed_h = np.concatenate([q_hashes, extra])
    feed_c = np.concatenate([q_counts, np.full(len(extra), 3, np.uint32)])
    s = len(q_hashes) if len(extra) else 0
    pair_hash, pair_gen = np.asarray(pair_hash, dtype=np.uint64), np.asarray(pair_gen, dtype=np.uint32)
    assert np.all(pair_hash[:-1] <= pair_hash[1:]) and (len(pair_hash) == 0 or int(pair_hash[-1]) <= TOP)
    qh, qc, truncated, bound = effective_sketch(feed_h, feed_c, s, set_bound)
    gsize = np.bincount(pair_gen.astype(np.int64), minlength=ngenomes).astype(np.uint32)
    return Case(name, feed_h, feed_c, s, set_bound, qh, qc, truncated, bound, pair_hash, pair_gen, gsize, ngenomes)


def _distinct(rng, lo, hi, n):
    """n distinct hashes in [lo, hi], ascending."""
    if n == 0:
        return np.zeros(0, np.uint64)
    assert hi - lo + 1 >= 2 * n
    got = np.zeros(0, np.uint64)
    while len(got) < n:
        got = np.unique(np.concatenate([got, rng.integers(lo, hi, size=n + 64, dtype=np.uint64, endpoint=True)]))
    return np.sort(rng.permutation(got)[:n])


def _sorted_pairs(rng, hashes, ngenomes, gens=None):
    """Pairs in hash order; genomes drawn from `gens` (default: all)."""
    hashes = np.asarray(hashes, dtype=np.uint64)
    order = np.argsort(hashes, kind="stable")
    g = rng.choice(np.arange(ngenomes) if gens is None else np.asarray(gens), size=len(hashes)).astype(np.uint32)
    return hashes[order], g[order]


# ================================================================ the families ==================================================
RUN_LENGTHS = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000]
RUN_SHIFT = 53  # (what plan_index gives the sketch of run_lengths(): ~15 k entries, 2048 buckets, a last hash of 64 bits)


def run_span(t, length):
    """[lo, hi]: the buckets' hash range that tile t of run_lengths() and its part of the sketch have to themselves."""
    b0, w = 100 + 140 * t, 1 if length <= 2 else 4
    return b0 << RUN_SHIFT, ((b0 + w) << RUN_SHIFT) - 1


@functools.lru_cache(maxsize=None)
def run_lengths():
    """One table of thirteen whole tiles; tile t's pairs and exactly RUN_LENGTHS[t] sketch entries lie in a span of buckets of
    their own, so tile t's run has that length.  Sketch entries are multiples of 4 inside the span: hash +- 1 of one is absent."""
    rng = np.random.default_rng(20261)
    ngen = 40
    qh, qc, ph = [], [], []
    for t, length in enumerate(RUN_LENGTHS):
        lo, hi = run_span(t, length)
        run = U64(lo) + U64(4) * _distinct(rng, 1, (hi - lo) // 4 - 1, length)
        cnt = rng.integers(0, 4, size=length).astype(np.uint32)  # counts on either side of every ci
        cnt[:1], cnt[-1:] = 3, 3                                  # the run's first and last entry match at every ci
        tile = [u64([lo + 1, hi - 1])]                            # first and last pair: in the span's first and last bucket, absent
        if length:
            near = run[rng.permutation(length)[:150]]
            tile += [run[[0, 0, -1, -1]], run[rng.permutation(length)[:500]], near + U64(1), near - U64(1)]
        have = sum(len(x) for x in tile)
        tile.append(rng.integers(lo + 2, hi - 2, size=KCTILE - have, dtype=np.uint64))
        qh.append(run)
        qc.append(cnt)
        ph.append(np.sort(np.concatenate(tile)))
    pair_hash, pair_gen = _sorted_pairs(rng, np.concatenate(ph), ngen)
    return [_case("thirteen run lengths", np.concatenate(qh), np.concatenate(qc), pair_hash, pair_gen, ngen)]


TILE_NPAIRS = [1, 255, 256, 257, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097] + [900, 1124, 1536, 1537, 3348]
EMPTY_GENOMES = [0, 1] + list(range(20, 30)) + [58, 59]  # first, in a run, last
SHARED = 5000  # genomes that share one hash


@functools.lru_cache(maxsize=None)
def tile_edges():
    rng = np.random.default_rng(20262)
    out = []
    ngen = 60
    used = [g for g in range(ngen) if g not in EMPTY_GENOMES]
    for npairs in TILE_NPAIRS:
        ph, pg = _sorted_pairs(rng, rng.integers(1 << 20, TOP, size=npairs, dtype=np.uint64, endpoint=True), ngen, used[:-1])
        pg[-1] = used[-1]              # the last pair is that genome's only one, and it is a match
        if npairs >= 4:                # a pair listed twice counts twice
            m = npairs // 2
            ph[m + 1], pg[m + 1] = ph[m], pg[m]
        present = np.unique(np.concatenate([ph[rng.random(npairs) < 0.5], ph[:1], ph[-1:]]))
        other = rng.integers(0, TOP, size=len(present), dtype=np.uint64, endpoint=True)
        qh = np.unique(np.concatenate([present, other]))
        qc = rng.integers(0, 4, size=len(qh)).astype(np.uint32)
        qc[np.searchsorted(qh, ph[[0, -1]])] = 3
        out.append(_case("npairs=%d" % npairs, qh, qc, ph, pg, ngen))
    out.append(_case("no pairs", u64([5, 9, TOP]), [3, 3, 3], [], [], 4))
    # one hash shared by 5000 genomes: whole tiles of it
    ngen = SHARED + 200
    below = rng.integers(1 << 20, 1 << 62, size=700, dtype=np.uint64)
    above = rng.integers((1 << 62) + 2, TOP, size=300, dtype=np.uint64, endpoint=True)
    shared = 1 << 62
    ph = np.sort(np.concatenate([below, np.full(SHARED, shared, np.uint64), above]))
    pg = rng.integers(0, ngen, size=len(ph)).astype(np.uint32)
    pg[700: 700 + SHARED] = np.arange(100, 100 + SHARED)
    rest = np.unique(np.concatenate([below[::2], above[::2], rng.integers(0, TOP, size=300, dtype=np.uint64)]))
    rest = rest[rest != U64(shared)]
    rc = rng.integers(0, 4, size=len(rest)).astype(np.uint32)
    for name, count in (("present", 3), ("absent", None), ("present below ci", 1)):
        qh, qc = rest, rc
        if count is not None:
            at = int(np.searchsorted(rest, U64(shared)))
            qh, qc = np.insert(rest, at, U64(shared)), np.insert(rc, at, count)
        out.append(_case("one hash in %d genomes, %s" % (SHARED, name), qh, qc, ph, pg, ngen))
    return out


SMALL_N = [1, 2, 7, 8, 9, 16, 17]


def _around(hashes, shift, buckets):
    """Table hashes for a small sketch: every sketch hash and its neighbours, every bucket border and the hash below it."""
    t = set()
    for h in hashes:
        t |= {int(h) - 1, int(h), int(h) + 1}
    for b in range(1, buckets + 1):
        t |= {(b << shift) - 1, b << shift}
    return sorted(x for x in t if 0 <= x <= TOP)


@functools.lru_cache(maxsize=None)
def hash_edges():
    rng = np.random.default_rng(20263)
    out = []
    ngen = 5
    # ---- the smallest sketches, the largest and the smallest hashes
    special = [TOP, 0, 1 << 63, (1 << 63) - 1, 1 << 62, (1 << 62) - 1, 3 << 62]
    fill = [k * ((1 << 64) // 19) + 5 for k in range(1, 18)]
    sketches = [("n=%d" % n, sorted((special + fill)[:n])) for n in SMALL_N]
    sketches += [("n=1, hash 0", [0]), ("n=1, hash 2^63", [1 << 63]), ("n=2, hashes 0 and 1", [0, 1])]
    for name, hs in sketches:
        qh = u64(hs)
        qc = (3 - (np.arange(len(qh)) % 4)).astype(np.uint32)
        qc[[0, -1]] = 3
        shift, buckets = plan_index(qh)
        ph = u64(_around(hs, shift, buckets) * 2)
        ph, pg = _sorted_pairs(rng, ph, ngen)
        out.append(_case(name, qh, qc, ph, pg, ngen))
    # ---- a sketch of 40-bit hashes: a table hash above it would index far behind the bucket index
    ngen = 12
    for n, name in ((3000, "staged"), (6000, "per pair")):
        qh = _distinct(rng, 1 << 39, (1 << 40) - 1, n)
        qc = rng.integers(0, 4, size=n).astype(np.uint32)
        qc[-1] = 3
        q_last = int(qh[-1])
        if name == "staged":
            ph, pg = _sorted_pairs(rng, rng.integers(0, (1 << 39) - 1, size=2500, dtype=np.uint64), ngen)
            out.append(_case("table below the sketch", qh, qc, ph, pg, ngen))
            ph, pg = _sorted_pairs(rng, rng.integers(1 << 40, TOP, size=2500, dtype=np.uint64, endpoint=True), ngen)
            out.append(_case("table above the sketch", qh, qc, ph, pg, ngen))
        first = int(qh[-500]) if name == "staged" else int(qh[100])
        inside = qh[qh >= U64(first)]
        low = [u64([first, q_last, q_last, q_last - 1, q_last + 1, q_last + 1, q_last + 2]), inside[rng.permutation(len(inside))[:700]],
               rng.integers(first, q_last, size=500, dtype=np.uint64)]
        have = sum(len(x) for x in low)
        high = rng.integers(q_last + 1, TOP, size=KCTILE + 500 - have, dtype=np.uint64, endpoint=True)  # the tile straddles q_last
        ph, pg = _sorted_pairs(rng, np.concatenate(low + [high]), ngen)
        out.append(_case("a tile straddles the last hash, %s" % name, qh, qc, ph, pg, ngen))
    # ---- hashes on bucket borders: b << shift and (b << shift) - 1, in the sketch and as the first / last pair of a tile
    shift = 54  # (6000 entries, a last hash of 64 bits: 1024 buckets)
    borders = [b << shift for b in range(1, 1024)] + [(b << shift) - 1 for b in range(1, 1024)] + [TOP]
    qh = np.unique(np.concatenate([u64(borders), rng.integers(0, TOP, size=6000 - len(borders), dtype=np.uint64)]))
    qc = rng.integers(0, 4, size=len(qh)).astype(np.uint32)
    qc[np.searchsorted(qh, u64([10 << shift, (40 << shift) - 1, 100 << shift, (600 << shift) - 1, TOP]))] = 3
    tiles = []
    for b0, b1, size in ((10, 40, KCTILE), (100, 600, KCTILE), (1000, 1024, 300)):
        edge = [b << shift for b in range(b0, b1)] + [(b << shift) - 1 for b in range(b0 + 1, b1 + 1)]
        off = [(b << shift) + 1 for b in range(b0, b1, 2)] + [(b << shift) - 2 for b in range(b0 + 1, b1 + 1, 2)]
        t = [min(x, TOP) for x in edge + off]
        t += rng.integers(b0 << shift, min((b1 << shift) - 1, TOP), size=size - len(t), dtype=np.uint64, endpoint=True).tolist()
        tiles.append(np.sort(u64(t)))
    ph, pg = _sorted_pairs(rng, np.concatenate(tiles), ngen)
    out.append(_case("bucket borders", qh, qc, ph, pg, ngen))
    # ---- thousands of empty buckets between two clusters: one thread of k_build_index fills them all
    shift = 52  # (20000 entries, 64 bits: 4096 buckets)
    qh = np.concatenate([_distinct(rng, 0, (40 << shift) - 1, 10000), _distinct(rng, 4000 << shift, TOP, 10000)])
    qc = rng.integers(0, 4, size=len(qh)).astype(np.uint32)
    low, high = qh[:10000], qh[10000:]
    t1 = np.concatenate([low[5000:5600], low[5000:5200] + U64(1), rng.integers(int(low[5000]), int(low[5600]), size=KCTILE - 800, dtype=np.uint64)])
    t2 = rng.integers(1000 << shift, 3000 << shift, size=KCTILE, dtype=np.uint64)
    t3 = np.concatenate([rng.integers(3900 << shift, (4000 << shift) - 1, size=1200, dtype=np.uint64), high[:400],
                         rng.integers(4000 << shift, int(high[500]), size=KCTILE - 1600, dtype=np.uint64)])
    t4 = np.concatenate([high[-300:], high[-100:] + U64(1), u64([TOP] * 3)])
    t4 = np.minimum(t4, U64(TOP))
    for t in (t1, t2, t3):
        assert len(t) == KCTILE
    assert t1.max() < t2.min() and t2.max() < t3.min() and t3.max() < t4.min()
    ph, pg = _sorted_pairs(rng, np.concatenate([t1, t2, t3, t4]), ngen)
    out.append(_case("a gap of empty buckets", qh, qc, ph, pg, ngen))
    return out


CROSS = (2040, 2061)  # positions [a, b) of the hash whose equal run crosses the first tile boundary in bounds()


@functools.lru_cache(maxsize=None)
def bounds():
    """Truncated sketches against one table of 5000 pairs (three tiles, the last ragged)."""
    rng = np.random.default_rng(20264)
    ngen = 30
    a = _distinct(rng, 1 << 20, TOP - 2, 5000 - (CROSS[1] - CROSS[0]) + 1)
    ph = np.concatenate([a[:CROSS[0]], np.full(CROSS[1] - CROSS[0] - 1, a[CROSS[0]], np.uint64), a[CROSS[0]:]])
    pg = rng.integers(0, ngen, size=len(ph)).astype(np.uint32)
    pg[CROSS[0]:CROSS[1]] = np.arange(CROSS[1] - CROSS[0])  # (the run: one pair per genome)
    cross = int(ph[CROSS[0]])
    assert len(ph) == 5000 and int(ph[CROSS[0] - 1]) < cross == int(ph[CROSS[1] - 1]) < int(ph[CROSS[1]])
    inside = np.unique(ph[rng.random(len(ph)) < 0.4])
    qh_all = np.unique(np.concatenate([inside, rng.integers(1 << 20, TOP - 2, size=1500, dtype=np.uint64), u64([cross, int(ph[-1]), int(ph[4095])])]))
    qc_all = rng.integers(0, 4, size=len(qh_all)).astype(np.uint32)
    qc_all[np.searchsorted(qh_all, u64([cross, int(ph[-1]), int(ph[4095])]))] = 3

    def upto(h, strict=False):
        keep = qh_all < U64(h) if strict else qh_all <= U64(h)
        return qh_all[keep], qc_all[keep], qh_all[~keep]

    out = []
    qh, qc, rest = upto(cross)
    out.append(_case("s: the bound is the hash whose run crosses a tile boundary", qh, qc, ph, pg, ngen, extra=rest))
    low = u64(range(7, 7 + 50 * 11, 11))
    out.append(_case("s: the bound lies below the first pair", low, np.full(50, 3, np.uint32), ph, pg, ngen, extra=qh_all[:20]))
    qh, qc, rest = upto(int(ph[4095]))
    out.append(_case("s: the bound is the last pair of the second tile", qh, qc, ph, pg, ngen, extra=rest))
    qh, qc, rest = upto(int(ph[-1]))
    out.append(_case("s: the bound is the table's last hash", qh, qc, ph, pg, ngen, extra=u64([TOP - 1, TOP])))
    assert int(ph[3001]) - int(ph[3000]) > 1
    qh, qc, _ = upto(int(ph[3000]))
    out.append(_case("set_bound: between two hashes", qh, qc, ph, pg, ngen, set_bound=(True, int(ph[3000]) + 1)))
    out.append(_case("set_bound: above the table", qh_all, qc_all, ph, pg, ngen, set_bound=(True, TOP)))
    qh, qc, _ = upto(cross, strict=True)
    out.append(_case("set_bound: the crossing hash, the sketch ends below it", qh, qc, ph, pg, ngen, set_bound=(True, cross)))
    out.append(_case("set_bound: below the first pair", low, np.full(50, 3, np.uint32), ph, pg, ngen, set_bound=(True, int(ph[0]) - 1)))
    out.append(_case("set_bound: an empty sketch", [], [], ph, pg, ngen, set_bound=(True, int(ph[2500]))))
    qh, qc, _ = upto(int(ph[3000]))
    out.append(_case("set_bound: not truncated", qh, qc, ph, pg, ngen, set_bound=(False, int(ph[100]))))
    return out


# 512 / 513 do not straddle a step of the rule (64 copies up to 1024 genomes); 1024 / 1025 do (64 -> 32), and 32768 / 32769 (2 -> 1)
COPIES_GENOMES = [1, 2, 512, 513, 1024, 1025, 32768, 32769]
HOT = 3000  # pairs of one genome that the sketch holds


@functools.lru_cache(maxsize=None)
def copies_cases():
    rng = np.random.default_rng(20265)
    out = []
    for ngen in COPIES_GENOMES:
        hot = [ngen // 2, ngen - 1]
        hs = _distinct(rng, 1 << 20, TOP, 2 * HOT + 2500)
        pg = rng.integers(0, ngen, size=len(hs)).astype(np.uint32)
        where = rng.permutation(len(hs))
        pg[where[:HOT]], pg[where[HOT:2 * HOT]] = hot[0], hot[1]
        present = np.zeros(len(hs), dtype=bool)
        present[where[:2 * HOT]] = True
        present[where[2 * HOT:]] = rng.random(2500) < 0.5
        qh = np.unique(np.concatenate([hs[present], rng.integers(0, TOP, size=1000, dtype=np.uint64)]))
        qc = rng.integers(1, 4, size=len(qh)).astype(np.uint32)
        out.append(_case("G=%d" % ngen, qh, qc, hs, pg, ngen))
    return out


FAMILIES = {"run_lengths": run_lengths, "tile_edges": tile_edges, "hash_edges": hash_edges, "bounds": bounds, "copies": copies_cases}


def case(family, name):
    return {c.name: c for c in FAMILIES[family]()}[name]


# Several cases in ONE containment_multi_dev call: a neighbour without a tile first, in the middle and last; a truncated sketch
# beside untruncated ones; tables whose genome counts ask for different numbers of counter copies (the largest decides)
MULTI = {
    "zero tiles in the middle": [("run_lengths", "thirteen run lengths"), ("bounds", "s: the bound lies below the first pair"),
                                 ("tile_edges", "npairs=2049"), ("copies", "G=1")],
    "zero tiles first, one counter copy": [("tile_edges", "no pairs"), ("bounds", "s: the bound is the hash whose run crosses a tile boundary"),
                                           ("hash_edges", "bucket borders"), ("copies", "G=32769")],
    "zero tiles last": [("hash_edges", "n=1, hash 0"), ("tile_edges", "one hash in 5000 genomes, present"),
                        ("hash_edges", "table above the sketch"), ("bounds", "set_bound: below the first pair")],
    "truncated beside untruncated": [("bounds", "set_bound: between two hashes"), ("tile_edges", "npairs=4097"),
                                     ("bounds", "set_bound: an empty sketch"), ("hash_edges", "a tile straddles the last hash, per pair")],
}


# ================================================================ the reference pipeline's table ================================
RefCase = namedtuple("RefCase", "name ks ngenomes pair_hash pair_gen gsize small q_hashes q_counts kmer_hi kmer_lo head")


def count_list(pa, pair_gen, ngenomes):
    """The table's own rule (mg_refdb_build): the distinct (prefix number, genome) combinations of the pairs' kept strand, ascending,
    and per genome how many there are."""
    key = np.unique((np.asarray(pa, dtype=np.uint64) << U64(32)) | np.asarray(pair_gen, dtype=np.uint64))
    cid, cgen = (key >> U64(32)).astype(np.uint32), (key & U64(0xFFFFFFFF)).astype(np.uint32)
    return cid, cgen, np.bincount(cgen.astype(np.int64), minlength=ngenomes).astype(np.uint32)


def _kmers(rng, npairs, shared):
    """Hand-made 21-mers, 'A' + 19 bases + 'A' (the forward strand is the canonical one, so distinct values are distinct k-mers);
    pair j of `shared` holds the k-mer of the pair before it.  -> (kmer_hi, kmer_lo, head): head[i] = first pair with i's k-mer."""
    mid = _distinct(rng, 0, (1 << 38) - 1, npairs)[rng.permutation(npairs)]
    for j in shared:
        mid[j] = mid[j - 1]
    lo = mid << U64(2)
    first = {}
    head = np.array([first.setdefault(int(v), i) for i, v in enumerate(lo)], dtype=np.uint32)
    return np.zeros(npairs, np.uint64), lo, head


def _refcase(rng, name, ks, ngenomes, npairs, nprefix, dups, match=0.1):
    """pair i: genome i % G, prefix number i // G on the kept strand (so every (prefix, genome) is distinct), except that pairs
    G .. G + dups[s] - 1 of small k number s repeat the prefix of the pair G places before them: ncount = npairs - dups[s]."""
    ph = _distinct(rng, 1 << 20, TOP, npairs)
    pg = (np.arange(npairs) % ngenomes).astype(np.uint32)
    small = []
    for s, (npre, d) in enumerate(zip(nprefix, dups)):
        pa = (np.arange(npairs) // ngenomes).astype(np.uint32)
        assert npairs == 0 or int(pa.max()) <= npre - 1
        if npairs:
            pa[pa == pa.max()] = npre - 1                                # the last bit of the bitmap is in the count list
        assert d <= ngenomes
        for j in range(ngenomes, ngenomes + d):
            pa[j] = pa[j - ngenomes]
        pb = rng.integers(0, npre, size=npairs).astype(np.uint32)
        kinds = rng.integers(0, 8, size=npairs)
        pb[kinds == 0] = NONE
        pb[kinds == 1] = pa[kinds == 1]
        pb[kinds == 2] = 40                                              # one prefix marked by many pairs
        edge = np.array([0, 31, 32, 63, npre - 1], dtype=np.uint32)      # the bits either side of a word of the bitmap
        pick = kinds == 3
        pb[pick] = edge[rng.integers(0, 5, size=int(pick.sum()))]
        cid, cgen, gs = count_list(pa, pg, ngenomes)
        small.append(dict(pa=pa, pb=pb, cid=cid, cgen=cgen, gsize=gs, nprefix=npre))
    present = ph[rng.random(npairs) < match]
    qh = np.unique(np.concatenate([present, rng.integers(0, TOP, size=200, dtype=np.uint64)]))
    qc = rng.integers(1, 4, size=len(qh)).astype(np.uint32)
    shared = [j for j in range(3, npairs, 7)]
    khi, klo, head = _kmers(rng, npairs, shared)
    gsize = np.bincount(pg.astype(np.int64), minlength=ngenomes).astype(np.uint32)
    return RefCase(name, ks, ngenomes, ph, pg, gsize, small, qh, qc.astype(np.uint32), khi, klo, head)


@functools.lru_cache(maxsize=None)
def refpipe():
    rng = np.random.default_rng(20266)
    return [
        # count lists of 2047, 2048 and 2049 entries: the second k starts one entry before a tile edge, the third on one
        _refcase(rng, "count lists of 2047, 2048, 2049", [5, 9, 13, 21], 8, 2049, [257, 300, 1000], [2, 1, 0]),
        # 4096 and 4100: the second k starts on a tile edge and ends in a ragged tile
        _refcase(rng, "count lists of 4096 and 4100", [7, 11, 21], 5, 4100, [821, 2000], [4, 0], match=0.04),
        _refcase(rng, "one pair", [9, 21], 3, 1, [65], [0], match=1.0),
        _refcase(rng, "no pairs", [5, 9, 21], 3, 0, [1, 33], [0, 0]),
    ]


REFPIPE_WORLDS = [2, 3, 5]  # set_count_share: runs of the count lists that begin and end inside tiles


def counters(rc, ci, cs, seed=0):
    """Hand-made stage-A counters for the by-identity path: u32[npairs] over {0, ci - 1, ci, cs, cs + 1, 0xffffffff}.  Only the
    counter at a pair's head is read; the others hold values that would change the answer if they were."""
    rng = np.random.default_rng(1000 * ci + 10 * cs + seed)
    values = np.array([0, ci - 1, ci, cs, cs + 1, 0xFFFFFFFF], dtype=np.uint32)
    return values[rng.integers(0, len(values), size=len(rc.pair_hash))]


def oracle_table(rc):
    """The dict oracle.refpipe_containment takes."""
    return dict(ks=list(rc.ks), ngenomes=rc.ngenomes, pair_hash=rc.pair_hash, pair_gen=rc.pair_gen, gsize=rc.gsize,
                small={k: t for k, t in zip(rc.ks[:-1], rc.small)})
