"""Stage C's chained scan (k_profile_pass, k_bins_reduce; metalign_amd/csrc/mg_profile.hip) held to its definition at every tile,
window, halo, flush and hash edge: record streams built BY POSITION (test infrastructure, no device needed).

  * the whole-stream definition is oracle.profile_assign (the C oracle pinned to the reference's golden vectors);
  * per read and per shard it is tests/shard_ref.run_shard, sequential Python (cases of at most PY_LIMIT records);
  * model() restates the kernel's GEOMETRY from the constants below alone — where a read leads, whether the line that closes it
    is staged, which reads need the set intersection, every thread's and tile's 2-bit state map, the tile counters, the hashed
    table's probe sequence — so that tests/test_profile_cases_host.py can prove each case reaches the edge it is named after.
    test_profile_cases_host.py reads the constants back from the source text: a changed constant fails there.

The four state maps, each realised by ONE read (bit x of a map = the state the read leaves when it is entered with state x;
1 = "first line dropped"):  identity = one kept line;  constant-kept = lines flagged 0 + 256;  constant-dropped = one rejected
line;  swap = lines flagged 65 + 129 on two taxa, closed by a paired line."""
import functools
from collections import namedtuple

import numpy as np

import shard_ref
from oracle import REC_DTYPE

# ---- the kernel's constants (read back from mg_profile.hip by the host test)
PB, ITEMS, HALO, WIN, TICKET_LANES = 256, 8, 64, 4, 16
TILE, STAGED, WIN_TILES = PB * ITEMS, PB * ITEMS + HALO, 64 * WIN
HASH_SLOTS, HASH_PROBE, HASH_PROBE_FREE, HASH_CROWDED = 2048, 8, 64, 2048 * 3 // 4
FLUSH_TILES, HASH_FLUSH_TILES, HASH_MAX_TAX, QUEUE_LEN_BITS = 256, 15, (1 << 18) - 2, 14
HASH_MULT, DIRECT_MAX_TAX, LDS_TWO_PER_CU = 2654435761, 4096, 40 * 1024
HASH_COUNT_BITS, HASH_BASES_BITS, TILE_COUNTER_BITS = 15, 31, 13
QLIM = 1 << QUEUE_LEN_BITS
PY_LIMIT = 50_000      # records: the sequential Python definition is used up to here
PCT_ID = 0.5
M_DROP, M_SWAP, M_IDENT, M_KEEP = 3, 1, 2, 0   # constant-dropped, swap, identity, constant-kept

Case = namedtuple("Case", "name family recs ref2tax ntax knobs cuts marks twice shard_args")


# ---------------------------------------------------------------- streams by position
class Stream:
    """Records appended read by read; self.n is the index the next line gets.  marks[name] = index of a read's first line."""

    def __init__(self, ntax):
        self.ntax, self.n, self.parts, self.marks, self.want_paired = ntax, 0, [], {}, False

    def _add(self, ref, flag, length, ok, new):
        k = len(ref)
        part = np.zeros(k, dtype=REC_DTYPE)
        part["ref_new"] = (np.asarray(ref, dtype=np.int64) % self.ntax).astype(np.uint32) | (np.asarray(new, dtype=np.uint32) << 31)
        part["total"] = 100
        part["matched"] = np.where(np.broadcast_to(ok, k), 100, 10)   # 0.1 < PCT_ID: rejected by filter_line
        part["flag_len"] = np.broadcast_to(flag, k).astype(np.uint32) | (np.broadcast_to(length, k).astype(np.uint32) << 12)
        paired = bool(part["flag_len"][0] & 1) and bool(part["flag_len"][0] & 192)
        assert not self.want_paired or paired, "the read before this one is closed by a paired line"
        self.want_paired = False
        self.parts.append(part)
        self.n += k

    def read(self, ref, flag, length=100, ok=True, mark=None):
        """One read of len(ref) lines."""
        if mark:
            self.marks[mark] = self.n
        new = np.zeros(len(ref), dtype=np.uint32)
        new[0] = 1
        self._add(ref, flag, length, ok, new)

    def ones(self, count, first_tax=0, length=100, flag=0, span=None):
        """`count` identity reads (one kept line each) on taxa first_tax, first_tax + 1, ... (mod span, the taxonomy by default)."""
        if count > 0:
            self._add((first_tax + np.arange(count)) % (span or self.ntax), flag, length, True, np.ones(count, dtype=np.uint32))

    def same(self, count, t, length=100):
        """`count` identity reads on taxon t."""
        if count > 0:
            self._add(np.full(count, t), 0, length, True, np.ones(count, dtype=np.uint32))

    def fill_to(self, pos, span=None):
        assert pos >= self.n, (pos, self.n)
        self.ones(pos - self.n, first_tax=self.n % (span or self.ntax), span=span)

    def copy(self):
        c = Stream(self.ntax)
        c.n, c.parts, c.marks, c.want_paired = self.n, list(self.parts), dict(self.marks), self.want_paired
        return c

    # the four maps, and reads whose multimapped count depends on the state without the map doing so
    def one(self, t, length=100, flag=0, mark=None):
        self.read([t], flag, length, mark=mark)

    def rejected(self, t=0, mark=None):
        self.read([t], 0, 100, ok=False, mark=mark)

    def const_kept(self, t1, t2, mark=None, paired_close=False):
        """paired_close: the form that is constant-kept when a PAIRED line closes it (both mates on one taxon; flags 0 + 256 closed
        by a paired line are Ambiguous entered kept: a swap)."""
        if paired_close:
            self.read([t1, t1], [65, 129], mark=mark)
        else:
            self.read([t1, t2], [0, 256], mark=mark)

    def swap(self, ta, tb, mark=None):
        self.read([ta, tb], [65, 129], mark=mark)
        self.want_paired = True

    def ident_mm(self, t, mark=None):
        """Identity map; entered kept it is multimapped (two lines, one of them rejected), entered dropped Ambiguous."""
        self.read([t, t + 1], 0, 100, ok=[True, False], mark=mark)

    # long reads of n lines, closed by the next read's first line
    def long_uniq(self, n, t, mark=None):
        """Single end (closed by an unpaired line), unique either way: on taxon t entered kept, t + 1 entered dropped."""
        self.read(t + np.arange(n), [0] + [129] * (n - 1), mark=mark)

    def long_mm(self, n, t, mark=None):
        """Single end, multimapped: n list entries entered kept, n - 1 entered dropped."""
        self.read(t + np.arange(n), [0] + [256] * (n - 1), mark=mark)

    def long_pair(self, n, t, mark=None):
        """Both mates mapped (classify == 3): taxa t, t + 1 alternate; two mate-1 lines, then mate-2 lines.  Entered kept the
        intersection holds both taxa (multimapped, n entries); entered dropped only t + 1 (unique)."""
        assert n >= 4
        self.read(t + (np.arange(n) & 1), [65, 65] + [129] * (n - 2), mark=mark)
        self.want_paired = True

    def done(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=REC_DTYPE)


def _case(name, family, s, knobs=(), cuts=((),), twice=False, shard_args=None, recs=None):
    recs = s.done() if recs is None else recs
    return Case(name, family, recs, np.arange(s.ntax, dtype=np.uint32), s.ntax, dict(knobs), tuple(tuple(c) for c in cuts),
                dict(s.marks), twice, shard_args)


def _tile_cuts(recs, tiles):
    """Cuts at read starts one record before, on and one record after the given tile multiples (where a read starts there)."""
    new = (recs["ref_new"] >> 31).astype(bool)
    return [p for t in tiles for p in (t * TILE - 1, t * TILE, t * TILE + 1) if 0 < p < len(recs) and new[p]]


# ---------------------------------------------------------------- the model of the kernel's geometry
def probe_slots(tax, n=HASH_PROBE_FREE):
    """The first n slots of the hashed table a taxon walks (double hashing over kHashSlots slots)."""
    hh = (tax * HASH_MULT) & 0xFFFFFFFF
    sl, stride = hh >> 21, ((hh >> 10) & 2046) | 1
    return [(sl + i * stride) & (HASH_SLOTS - 1) for i in range(n)]


def hist_mode(ntax, hashed_knob=False):
    """-> (use_lds_hist, workgroups per CU) as launch_pass decides them below 2^32 - 1 records."""
    mode = 1 if ntax <= DIRECT_MAX_TAX else 2 if ntax <= HASH_MAX_TAX else 0
    if mode == 1 and hashed_knob:
        mode = 2
    lds = 0 if mode == 0 else 12 * (ntax if mode == 1 else HASH_SLOTS)
    return mode, 2 if lds > LDS_TWO_PER_CU else 3


def compose(first, second):
    return ((second >> (first & 1)) & 1) | (((second >> ((first >> 1) & 1)) & 1) << 1)


def _compose_runs(maps, a, b):
    """The composed map of reads [a[i], b[i]) for every i (vectorised: the last constant map of a run decides, swaps after it flip)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = len(maps)
    is_const = (maps == M_KEEP) | (maps == M_DROP)
    sw = np.concatenate([[0], np.cumsum(maps == M_SWAP)]).astype(np.int64)
    last = np.maximum.accumulate(np.where(is_const, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    lastb = np.where(b > a, last[np.maximum(b - 1, 0)] if n else -1, -1)
    has = lastb >= a
    cval = np.where(has, (maps[np.maximum(lastb, 0)] if n else 0) & 1, 0)
    flips = (sw[b] - sw[np.where(has, lastb + 1, a)]) & 1
    f0 = np.where(has, cval, 0) ^ flips
    f1 = np.where(has, cval, 1) ^ flips
    return (f0 | (f1 << 1)).astype(np.int64), np.where(has, lastb, -1)


Model = namedtuple("Model", "starts lead tile close staged kinds nmm classify3 read_map thread_map tile_map state_in tile_state_in "
                            "decided_by kind nmm_true tile_reads tile_mm tile_entries ntiles shard_map")


def model(recs, ref2tax, nrecs=None, has_look=False, incoming=1, pct_id=PCT_ID):
    """The kernel's view of one shard: records [0, nrecs) owned, one lookahead record behind them when has_look.
    Per owned read (in order): starts (record index of its lead), lead (index within its tile), tile, close (record index of the
    line that closes it, -1: none), staged (that line is among the tile's nst staged descriptors), kinds[x] / nmm[x] (verdict and
    list entries entered with state x; -1 when never closed), classify3[x] (the counters do not decide: set intersection),
    read_map, state_in (true state entering it, from `incoming`), kind / nmm_true (the true verdict).
    Per thread / tile: thread_map[tile * PB + t], tile_map, tile_state_in, decided_by (the nearest earlier tile whose map is
    constant-through-its-last-constant-read, -1: the shard's incoming state), tile_reads / tile_mm / tile_entries (true path)."""
    nrecs = len(recs) - (1 if has_look else 0) if nrecs is None else nrecs
    ntotal = nrecs + (1 if has_look else 0)
    r = recs[:ntotal]
    fl = r["flag_len"] & 0xFFF
    new = (r["ref_new"] >> 31).astype(bool)
    a = ((fl & 1) != 0) & ((fl & 64) != 0)
    b = ((fl & 1) != 0) & ((fl & 128) != 0)
    rej = (r["matched"].astype(np.float64) / r["total"].astype(np.float64) < pct_id) | ((fl & 2048) != 0)
    p1c = (a | ~b).astype(np.int64) - (rej & a)
    p2c = b.astype(np.int64) - (rej & ~a & b)
    cs = lambda v: np.concatenate([[0], np.cumsum(v.astype(np.int64))])  # noqa: E731
    C1, C2, CK = cs(p1c), cs(p2c), cs(~rej)
    all_new = np.nonzero(new)[0]
    assert ntotal == 0 or new[0], "a shard starts at a read's first line"
    starts = all_new[all_new < nrecs]
    nreads = len(starts)
    close = np.full(nreads, -1, dtype=np.int64)
    k = min(nreads, len(all_new) - 1)
    close[:k] = all_new[1:k + 1]
    closed = close >= 0
    tile = starts // TILE
    lead = starts % TILE
    nst = np.minimum(ntotal - tile * TILE, STAGED)
    staged = closed & (close - tile * TILE < nst)
    end = np.where(closed, close, starts)
    npair = np.where(closed, (a | b)[np.maximum(close, 0)], False) if ntotal else np.zeros(0, bool)
    kinds, nmm, c3 = [], [], []
    lists = None
    for x in (0, 1):
        s = starts + x
        nk, p1, p2 = CK[end] - CK[np.minimum(s, end)], C1[end] - C1[np.minimum(s, end)], C2[end] - C2[np.minimum(s, end)]
        kd = np.where(nk == 0, 0, np.where(npair, np.where(p1 + p2 == 1, 1, np.where((p1 == 0) | (p2 == 0), 0, 3)), np.where(p1 > 1, 2, 1)))
        nm = np.where(kd == 2, nk, 0)
        three = closed & (kd == 3)
        for i in np.nonzero(three)[0]:  # the set intersection, read by read
            if lists is None:
                lists = {key: recs[key].tolist() for key in recs.dtype.names}
                r2t = np.asarray(ref2tax).tolist()
            kk, _, _, taxa = shard_ref._process(range(int(s[i]), int(close[i])), lists, r2t, pct_id, (True, True))
            kd[i], nm[i] = kk, len(taxa)
        kinds.append(np.where(closed, kd, -1))
        nmm.append(np.where(closed, nm, 0))
        c3.append(three)
    read_map = np.where(closed, (kinds[0] == 0) | ((kinds[1] == 0).astype(np.int64) << 1), M_IDENT).astype(np.int64)
    ntiles = (nrecs + TILE - 1) // TILE
    th = np.arange(ntiles * PB, dtype=np.int64) * ITEMS
    thread_map, _ = _compose_runs(read_map, np.searchsorted(starts, th), np.searchsorted(starts, th + ITEMS))
    t0 = np.arange(ntiles, dtype=np.int64) * TILE
    ta, tb = np.searchsorted(starts, t0), np.searchsorted(starts, t0 + TILE)
    tile_map, _ = _compose_runs(read_map, ta, tb)
    pre, _ = _compose_runs(read_map, np.zeros(nreads, np.int64), np.arange(nreads))
    state_in = (pre >> incoming) & 1
    tpre, tlast = _compose_runs(read_map, np.zeros(ntiles, np.int64), ta)
    tile_state_in = (tpre >> incoming) & 1
    decided_by = np.where(tlast >= 0, tile[np.maximum(tlast, 0)] if nreads else -1, -1)
    kind = np.where(state_in == 1, kinds[1], kinds[0])
    nmm_true = np.where(state_in == 1, nmm[1], nmm[0])
    cnt = lambda w: np.bincount(tile, weights=w, minlength=ntiles).astype(np.int64)  # noqa: E731
    shard_map, _ = _compose_runs(read_map, [0], [nreads])
    return Model(starts, lead, tile, close, staged, kinds, nmm, c3, read_map, thread_map, tile_map, state_in, tile_state_in,
                 decided_by, kind, nmm_true, cnt(np.ones(nreads)), cnt(kind == 2), cnt(np.where(kind == 2, nmm_true, 0)), ntiles,
                 (int(shard_map[0]) & 1, int(shard_map[0]) >> 1))


def shards(case, cuts):
    """-> [(records of the shard with its lookahead, nrecs, has_look)] for the stream cut at `cuts`."""
    bounds = [0] + list(cuts) + [len(case.recs)]
    out = []
    for lo, hi in zip(bounds, bounds[1:]):
        has_look = hi < len(case.recs)
        out.append((case.recs[lo:hi + (1 if has_look else 0)], hi - lo, has_look))
    return out


def define_shard(case, part, nrecs, has_look, incoming, first_shard, group_base):
    """The sequential Python definition of one shard (cases of at most PY_LIMIT records)."""
    assert len(case.recs) <= PY_LIMIT, case.name
    return shard_ref.run_shard(part, nrecs, has_look, case.ref2tax, case.ntax, PCT_ID, incoming, first_shard, group_base)


def mm_of(res):
    """run_shard's multimapped list -> (offsets, taxa, hitlen, read) as the library lays the CSR out."""
    off = np.zeros(len(res["mm"]) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(t) for _, t, _ in res["mm"]])
    tax = np.asarray([t for _, taxa, _ in res["mm"] for t in taxa], dtype=np.uint32)
    return off, tax, np.asarray([h for _, _, h in res["mm"]], dtype=np.uint64), np.asarray([r for r, _, _ in res["mm"]], dtype=np.uint64)


def verdict_words(res):
    """run_shard's verdicts -> the uint64[2 * reads] words of mg_profile_commit_assign_dev."""
    w = np.zeros(2 * len(res["verdicts"]), dtype=np.uint64)
    for i, (kind, tax, val) in enumerate(res["verdicts"]):
        w[2 * i] = kind | (tax << 2) if kind == 1 else kind
        w[2 * i + 1] = val
    return w


# ---------------------------------------------------------------- family 1: halo edges
HALO_LEADS = (0, 7, 8, 2040, 2046, 2047)
HALO_CLOSES = (STAGED - 2, STAGED - 1, STAGED, STAGED + 1)   # staged index of the closing line: 2110 .. 2113
HALO_FAR = (3000, 5000)                                      # ... and reads of so many lines
HALO_KINDS = ("uniq", "mm", "pair")


def _halo_stream(lead, kind, dropped):
    s = Stream(7)
    s.const_kept(1, 2)
    tile = 1
    for c in HALO_CLOSES + tuple(lead + n for n in HALO_FAR):
        base = tile * TILE
        s.fill_to(base + lead - (1 if dropped else 2))
        if dropped:
            s.rejected(3)
        else:
            s.const_kept(3, 4, paired_close=kind == "pair")
        assert s.n == base + lead
        getattr(s, "long_" + kind)(c - lead, s.n % 5, mark="close%d" % c if c < 3000 else "far%d" % (c - lead))
        s.one(5, flag=65 if kind == "pair" else 0)
        tile = (s.n + 2 + TILE - 1) // TILE
    s.fill_to(tile * TILE + 5)
    return s


def halo_edges():
    out = []
    for lead in HALO_LEADS:
        for kind in HALO_KINDS:
            for dropped in (False, True):
                s = _halo_stream(lead, kind, dropped)
                recs = s.done()
                out.append(_case("lead%d_%s_%s" % (lead, kind, "dropped" if dropped else "kept"), "halo_edges", s, recs=recs,
                                 cuts=((), _tile_cuts(recs, (1, 2)))))
    # the last tile: nrecs = 2048 m - 1, 2048 m, 2048 m + 1 (m = 2), the last read short (closed by a staged lookahead) or longer
    # than the halo (closed by the lookahead through the walk in HBM); the same streams END there in the "nolook" cases, where
    # the last read has no closing line and its verdict word stays 3
    for d in (-1, 0, 1):
        for nlast, tag in ((4, "short"), (2200, "long")):
            for kind in ("mm", "pair"):
                nrecs = 2 * TILE + d
                s = Stream(7)
                s.const_kept(1, 2)
                s.fill_to(nrecs - nlast - 2)
                s.const_kept(3, 4, paired_close=kind == "pair")
                getattr(s, "long_" + kind)(nlast, 2, mark="last")
                assert s.n == nrecs
                whole = s.copy()
                whole.one(5, flag=65 if kind == "pair" else 0)
                whole.ones(9, first_tax=1)
                name = "tail%+d_%s_%s" % (d, tag, kind)
                out.append(_case(name, "halo_edges", whole, cuts=((nrecs,), (nrecs, nrecs))))
                out.append(_case(name + "_nolook", "halo_edges", s))
    return out


# ---------------------------------------------------------------- family 2: thread and wavefront edges
EDGE_THREADS = (3, 63, 127, 191, 255)


def thread_and_wave_edges():
    s = Stream(11)
    s.const_kept(1, 2)
    # tile 1: a read that opens in record 7 of thread t and is closed by record 0 of thread t + 1 (the next tile for t = 255);
    # alternately rejected, so that the thread's map is not the identity
    pos = TILE
    for i, t in enumerate(EDGE_THREADS):
        s.fill_to(pos + ITEMS * t + 7)
        if i & 1:
            s.rejected(t, mark="next%d" % t)
        else:
            s.one(t, mark="next%d" % t)
    # tile 2: ... and reads of nine lines, closed by record 0 of thread t + 2 (record 8 of the next tile for t = 255)
    pos = 2 * TILE
    for t in EDGE_THREADS:
        s.fill_to(pos + ITEMS * t + 7)
        s.long_mm(ITEMS + 1, t, mark="skip%d" % t)
    # tile 4: 2048 single-line reads
    s.fill_to(4 * TILE)
    s.marks["singles"] = s.n
    s.ones(TILE, first_tax=3)
    # tile 6 is the inside of one read: no read opens in it
    s.fill_to(5 * TILE + 100)
    s.long_mm(2 * TILE, 4, mark="inside")
    # tile 8: 1024 two-line multimapped reads (the most a tile's mm_reads field sees)
    s.fill_to(8 * TILE)
    s.marks["pairs"] = s.n
    new = np.tile(np.array([1, 0], dtype=np.uint32), TILE // 2)
    s._add(np.arange(TILE) // 2, np.tile(np.array([0, 256]), TILE // 2), 100, True, new)
    s.ones(20, first_tax=2)
    recs = s.done()
    return [_case("edges", "thread_and_wave_edges", s, recs=recs, cuts=((), _tile_cuts(recs, (2, 4, 5, 8, 9))))]


# ---------------------------------------------------------------- family 3: state chains
CHAIN_TILES = (2, 255, 256, 257, 258, 511, 512, 513, 600)
PROBES = ((300, 1), (300, 255), (300, 256), (300, 257), (560, 520))   # (probe tile, distance of the deciding tile behind it)
GROUP_BASES = (0, 1, 2**32 - 1, 2**32, 2**40)


def _slow_read(s):
    """A read that keeps its tile busy for a while (a long set intersection): the tiles behind it publish their aggregates
    first, so that far tiles find aggregates, not prefixes, in their look-back windows."""
    s.long_pair(1500, 2)
    s.one(1, flag=65)


def _chain(ntiles, dropped):
    s = Stream(7)
    if dropped:
        s.rejected(3)
    else:
        s.const_kept(1, 2)
    n = ntiles * TILE
    # identity reads only: ones, and (every 16th) a read that is multimapped when entered kept, Ambiguous when dropped
    k = (n - s.n) // 17
    new = np.ones((k, 17), dtype=np.uint32)
    new[:, 16] = 0
    ok = np.ones((k, 17), dtype=bool)
    ok[:, 16] = False
    ref = (np.arange(k * 17) * 3) % 7
    s._add(ref, 0, 100, ok.reshape(-1), new.reshape(-1))
    s.fill_to(n)
    return s


def _mixed(ntiles, seed):
    """Every kind of read at random places: all four maps, multimapped lists, set intersections."""
    rng = np.random.default_rng(seed)
    s = Stream(23)
    s.const_kept(1, 2)
    while s.n < ntiles * TILE - 5100:
        k = int(rng.integers(0, 12))
        t = int(rng.integers(0, 23))
        if k < 4:
            s.ones(int(rng.integers(1, 200)), first_tax=t)
        elif k == 4:
            s.rejected(t)
        elif k == 5:
            s.const_kept(t, t + 1)
        elif k == 6:
            s.swap(t, t + 1)
            s.one(t + 2, flag=65)
        elif k == 7:
            s.ident_mm(t)
        elif k == 8:
            s.long_pair(int(rng.integers(4, 12)), t)
            s.one(t + 2, flag=65)
        elif k == 9:
            s.read(t + np.arange(3), [0, 256, 256])
        elif k == 10:
            s.ones(int(rng.integers(1000, 5000)), first_tax=t)
        else:
            s.read(t + np.arange(int(rng.integers(2, 70))), 16)
    s.fill_to(ntiles * TILE)
    return s


def state_chains():
    out = []
    for nt in CHAIN_TILES:
        for dropped in (False, True):
            out.append(_case("chain%d_%s" % (nt, "dropped" if dropped else "kept"), "state_chains", _chain(nt, dropped)))
    # no decision at all: the state entering the SHARD decides every read of every tile
    s = Stream(7)
    body = _chain(20, False)
    s.parts, s.n = [body.done()[2:]], 20 * TILE - 2
    out.append(_case("undecided", "state_chains", s, cuts=((), _tile_cuts(s.parts[0], (1, 7)))))
    # tiles whose aggregate maps are each of the four maps, in every order of two
    s = Stream(7)
    s.const_kept(1, 2)
    order = [M_IDENT, M_SWAP, M_SWAP, M_DROP, M_SWAP, M_KEEP, M_SWAP, M_IDENT, M_DROP, M_DROP, M_KEEP, M_KEEP, M_IDENT, M_KEEP,
             M_DROP, M_IDENT, M_SWAP, M_IDENT]
    for i, m in enumerate(order):
        s.fill_to((i + 1) * TILE + 100 + 8 * i)
        s.marks["map_tile%d" % (i + 1)] = m
        for part in {M_SWAP: "sss", M_DROP: "kd", M_KEEP: "dk", M_IDENT: "ss"}[m]:  # (threads' maps differ from their tile's)
            if part == "s":
                s.swap(2, 3)
                s.one(4, flag=65)
            elif part == "k":
                s.const_kept(1, 2)
            else:
                s.rejected(3)
            s.ones(11, first_tax=i)
    s.fill_to((len(order) + 1) * TILE + 9)
    recs = s.done()
    out.append(_case("tile_maps", "state_chains", s, recs=recs, cuts=((), _tile_cuts(recs, range(1, len(order), 3)))))
    # a constant-map tile at distance d behind a probe tile, identity tiles between them, the opposite state before it, and a
    # slow read in tile 1: the nearest deciding tile sits on either side of the look-back window's edge
    for probe, d in PROBES:
        for dropped in (False, True):
            s = Stream(7)
            if dropped:
                s.const_kept(1, 2)
            else:
                s.rejected(3)
            s.fill_to(TILE + 10)
            _slow_read(s)
            if not dropped:
                s.rejected(3)   # (the slow read leaves "kept")
            s.fill_to((probe - d) * TILE + 1000)
            s.marks["decider"] = s.n
            if dropped:
                s.rejected(3)
            else:
                s.const_kept(1, 2)
            k = ((probe + 2) * TILE - s.n) // 3
            new = np.tile(np.array([1, 1, 0], dtype=np.uint32), k)   # ones and ident_mm reads to the end
            s._add(np.arange(3 * k) % 5, 0, 100, np.tile(np.array([True, True, False]), k), new)
            s.fill_to((probe + 2) * TILE)
            out.append(_case("probe%d_d%d_%s" % (probe, d, "dropped" if dropped else "kept"), "state_chains", s))
    # incoming x first_shard x group_base through begin / commit: one shard of three tiles with every kind of read
    s = _mixed(3, 5)
    out.append(_case("shard_args", "state_chains", s,
                     shard_args=[(i, f, g) for i in (0, 1) for f in (0, 1) for g in GROUP_BASES]))
    return out


# ---------------------------------------------------------------- family 4: grids and tickets
GRIDS = (1, 2, 15, 16, 17, 33, 0)   # 0: the launcher's grid


def grid_and_tickets():
    out = []
    for nt in (40, 300):
        s = _mixed(nt, nt)
        recs = s.done()
        for g in GRIDS:
            out.append(_case("mixed%d_grid%d" % (nt, g), "grid_and_tickets", s, recs=recs, knobs={"k3_grid": g} if g else {},
                             cuts=((), _tile_cuts(recs, (1, nt // 2)))))
    return out


# ---------------------------------------------------------------- family 5: bin fields
def _one_taxon(ntiles, ntax, tax, lengths=(QLIM - 1,), first_two=True):
    s = Stream(ntax)
    if first_two:
        s.read([tax, tax], [0, 256], length=[0, lengths[0]])   # entered dropped: unique, SEQ length lengths[0]
    n = ntiles * TILE - s.n - 1
    s._add(np.full(n, tax), 0, np.resize(np.asarray(lengths), n), True, np.ones(n, dtype=np.uint32))
    s.one(tax + 1)
    return s


def bin_fields():
    out = []
    g1 = {"k3_grid": 1}
    out.append(_case("direct_257", "bin_fields", _one_taxon(FLUSH_TILES + 1, 5, 2), knobs=g1))
    for nt in (HASH_FLUSH_TILES + 1, 2 * HASH_FLUSH_TILES + 1):
        out.append(_case("hashed_knob_%d" % nt, "bin_fields", _one_taxon(nt, 5, 2), knobs=dict(g1, k3_hashed=1)))
        out.append(_case("hashed_natural_%d" % nt, "bin_fields", _one_taxon(nt, DIRECT_MAX_TAX + 1, DIRECT_MAX_TAX - 2), knobs=g1))
    # the same entered KEPT (a shard of its own): tile 0 holds 2048 reads too, the bin is as full as the fields allow at the flush
    for name, ntax, tax, kn in (("hashed_knob_full", 5, 2, dict(g1, k3_hashed=1)), ("hashed_natural_full", DIRECT_MAX_TAX + 1, 4000, g1)):
        s = _one_taxon(HASH_FLUSH_TILES + 2, ntax, tax, first_two=False)   # (16 tiles of closed reads: one interval and a tile)
        out.append(_case(name, "bin_fields", s, knobs=kn, shard_args=[(0, 0, 0), (0, 1, 2**32)]))
    # SEQ lengths 16383 / 16384 interleaved on one (even) taxon: every other read bypasses the queue
    for name, ntax, tax, kn in (("bypass_direct", 5, 2, {}), ("bypass_hashed", 5, 2, {"k3_hashed": 1}),
                                ("bypass_natural", DIRECT_MAX_TAX + 1, 4000, {})):
        out.append(_case(name, "bin_fields", _one_taxon(3, ntax, tax, lengths=(QLIM - 1, QLIM)), knobs=kn))
    # first seen: a taxon whose only read is the shard's read 0, one whose only read is the last closed read, one reached through a
    # read whose first line was dropped
    for name, kn in (("first_seen_direct", {}), ("first_seen_hashed", {"k3_hashed": 1})):
        s = Stream(40)
        s.read([30, 31], [0, 256], mark="read0")    # entered dropped (the phantom boundary): unique on taxon 31
        s.ones(3 * TILE, span=30)
        s.rejected(3)
        s.read([32, 33], [0, 256], mark="after_dropped")  # first line dropped: unique on taxon 33
        s.fill_to(5 * TILE + 7, span=30)
        s.one(34, mark="last")
        s.one(1)
        s.marks.update(t_first=31, t_dropped=33, t_last=34)
        out.append(_case(name, "bin_fields", s, knobs=kn))
    return out


# ---------------------------------------------------------------- family 6: histogram modes
MODE_NTAX = (1, 2048, 2049, 3413, 3414, 4096, 4097, HASH_MAX_TAX, HASH_MAX_TAX + 1)


def mode_edges():
    out = []
    for ntax in MODE_NTAX:
        s = Stream(ntax)
        s.const_kept(ntax - 1, 0)
        for i in range(60):
            s.ones(97, first_tax=0 if i & 1 else ntax - 40)
            s.one(ntax - 1, length=QLIM - 1)
            s.one(0, length=QLIM)
            s.const_kept(ntax - 1, 0)
            s.long_mm(5, ntax - 3)
            s.one(ntax - 1)
        s.fill_to(4 * TILE + 11)
        s.one(ntax - 1)
        s.one(0)
        out.append(_case("ntax%d" % ntax, "mode_edges", s))
    return out


# ---------------------------------------------------------------- family 7: collisions in the hashed table
@functools.lru_cache(maxsize=None)
def collision_plan():
    """At the smallest ntax > 4096 where they exist: a target taxon T with, for each of its first 64 probe slots (all different), a
    blocker — a taxon other than T whose FIRST probe is that slot.  -> dict(ntax, T, blockers[64])"""
    for ntax in range(DIRECT_MAX_TAX + 1, HASH_MAX_TAX):
        by_first = {}
        for t in range(ntax):
            by_first.setdefault(probe_slots(t, 1)[0], []).append(t)
        for T in range(ntax):
            slots = probe_slots(T)
            blockers = [next((t for t in by_first.get(sl, ()) if t != T), None) for sl in slots]
            if None not in blockers and len(set(slots)) == len(slots):
                return dict(ntax=ntax, T=T, blockers=blockers)
    raise AssertionError("no collision plan")


@functools.lru_cache(maxsize=None)
def six_plan():
    """The smallest ntax at which six taxa share one first slot.  -> dict(ntax, six)"""
    by_first = {}
    for t in range(HASH_MAX_TAX):
        v = by_first.setdefault(probe_slots(t, 1)[0], [])
        v.append(t)
        if len(v) == 6:
            return dict(ntax=max(t + 1, DIRECT_MAX_TAX + 1), six=v)
    raise AssertionError("no six taxa share a slot")


def table_after(taxa, max_probe=HASH_PROBE_FREE):
    """The hashed table after the taxa were seen one by one in this order.  -> ({slot: taxon}, [taxa that found no slot])"""
    table, over = {}, []
    for t in taxa:
        for sl in probe_slots(t, max_probe):
            if table.setdefault(sl, t) == t:
                break
        else:
            over.append(t)
    return table, over


def _blocked(nblock, crowd=0):
    """Tile 0: the blockers of T's first nblock probe slots (and `crowd` more taxa); tile 1: T, between reads of the blockers."""
    p = collision_plan()
    T, blockers = p["T"], p["blockers"]
    s = Stream(p["ntax"])
    s.const_kept(blockers[0], blockers[0])
    for b in blockers[:nblock]:
        s.same(2, b)
    for t in [t for t in range(p["ntax"]) if t != T][:crowd]:
        s.one(t)
    assert s.n < TILE
    s.marks["T"] = TILE + 5
    s.same(TILE + 5 - s.n, blockers[0])
    for i in range(40):
        s.one(T, length=100 + i)
        s.one(blockers[i % nblock])
    s.one(blockers[0])
    return s


def hash_collisions():
    g1 = {"k3_grid": 1}
    out = [_case("blocked64", "hash_collisions", _blocked(HASH_PROBE_FREE), knobs=g1, twice=True),
           _case("blocked63", "hash_collisions", _blocked(HASH_PROBE_FREE - 1), knobs=g1, twice=True),
           _case("crowded8", "hash_collisions", _blocked(HASH_PROBE, crowd=1800), knobs=g1, twice=True)]
    # six taxa sharing one first slot, tile j holding the (j mod 6)-th of them only: at the launcher's grid the workgroups' last tables
    # hold different keys in that slot, more than k_bins_reduce caches
    p = six_plan()
    s = Stream(p["ntax"])
    s.const_kept(1, 2)
    for j in range(SIX_TILES):
        n = (j + 1) * TILE - s.n
        s._add(np.where(np.arange(n) % 3 == 0, p["six"][j % 6], 7 + j), 0, 100 + j, True, np.ones(n, dtype=np.uint32))
    s.one(1)
    out.append(_case("six_keys", "hash_collisions", s, twice=True))
    return out


SIX_TILES = 200
FAMILIES = {"halo_edges": halo_edges, "thread_and_wave_edges": thread_and_wave_edges, "state_chains": state_chains,
            "grid_and_tickets": grid_and_tickets, "bin_fields": bin_fields, "mode_edges": mode_edges, "hash_collisions": hash_collisions}


@functools.lru_cache(maxsize=None)
def family(name):
    return {c.name: c for c in FAMILIES[name]()}


def case(fam, name):
    return family(fam)[name]


def names(fam):
    return list(family(fam))


# the names alone, without building a stream (test ids; the host test holds them to the builders)
NAMES = {
    "halo_edges": ["lead%d_%s_%s" % (lead, k, st) for lead in HALO_LEADS for k in HALO_KINDS for st in ("kept", "dropped")]
                  + ["tail%+d_%s_%s%s" % (d, tag, k, look) for d in (-1, 0, 1) for tag in ("short", "long") for k in ("mm", "pair")
                     for look in ("", "_nolook")],
    "thread_and_wave_edges": ["edges"],
    "state_chains": ["chain%d_%s" % (n, st) for n in CHAIN_TILES for st in ("kept", "dropped")] + ["undecided", "tile_maps"]
                    + ["probe%d_d%d_%s" % (p, d, st) for p, d in PROBES for st in ("kept", "dropped")] + ["shard_args"],
    "grid_and_tickets": ["mixed%d_grid%d" % (nt, g) for nt in (40, 300) for g in GRIDS],
    "bin_fields": ["direct_257"] + [n % nt for nt in (HASH_FLUSH_TILES + 1, 2 * HASH_FLUSH_TILES + 1) for n in ("hashed_knob_%d", "hashed_natural_%d")]
                  + ["hashed_knob_full", "hashed_natural_full", "bypass_direct", "bypass_hashed", "bypass_natural", "first_seen_direct",
                     "first_seen_hashed"],
    "mode_edges": ["ntax%d" % n for n in MODE_NTAX],
    "hash_collisions": ["blocked64", "blocked63", "crowded8", "six_keys"],
}
ALL = [(fam, name) for fam in FAMILIES for name in NAMES[fam]]
