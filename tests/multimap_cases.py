"""Shared by the --multimap_iterations tests (CPU and -m gpu): the hand example, seeded multimapped CSRs, alignment records that
make stage C produce a chosen CSR, and the definition evaluated in decimal."""
import decimal

import numpy as np

from metalign_amd import multimap as mmdef

NAN = float("nan")

# taxa A, B, C; reads {A,B}, {A,B}, {B,C}, {B,C}, 100 bases each (metalign_amd/multimap.py)
HAND_W0 = [300.0, 100.0, 100.0]
HAND_OFF = [0, 2, 4, 6, 8]
HAND_TAX = [0, 1, 0, 1, 1, 2, 1, 2]
HAND_HITLEN = [100, 100, 100, 100]
HAND_AFTER_1 = [450.0, 250.0, 200.0]
HAND_AFTER_2 = [300 + 900 / 7, 100 + 500 / 7 + 1000 / 9, 100 + 800 / 9]

# A read whose only kept taxon weighs 0.0 (read 3 = {0}, written twice; read 0 = {0, 3} with taxon 3 without an entry) is skipped: den == 0.0.  That is
# decided anew in every iteration — but under the rule itself a weight of exactly 0.0 never grows (in a read with den > 0 its share is
# 0 / den = 0, and w_i = w0 + extra_i = 0), so such a read stays out of every iteration of one run, while read 2 = {0, 1} goes on
# giving taxon 0 a share of exactly 0.0 (touched, unchanged).  The re-evaluation itself shows at the level of one step with other
# weights (multimap.step), which is how the tests pin it.
ZERO_W0 = [0.0, 50.0, 150.0, NAN]
ZERO_OFF = [0, 2, 4, 6, 8]
ZERO_TAX = [0, 3, 1, 2, 0, 1, 0, 0]
ZERO_HITLEN = [80, 100, 60, 40]


def as_lists(off, tax):
    return [[int(t) for t in tax[int(off[r]):int(off[r + 1])]] for r in range(len(off) - 1)]


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists])
    tax = np.array([t for x in lists for t in x], dtype=np.uint32)
    return off, tax


def random_csr(rng, T, nreads, maxlen=7, fractional=False):
    """-> off, tax, hitlen, w0 (NaN: no entry; some 0.0), genome_len.  Repeated taxa, reads left empty."""
    lens = rng.integers(0, maxlen, size=nreads)
    off = np.zeros(nreads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    tax = rng.integers(0, T, size=int(off[-1])).astype(np.uint32)
    hitlen = rng.integers(30, 151, size=nreads).astype(np.uint64)
    w0 = np.full(T, np.nan)
    for t in range(T):
        if rng.random() < 0.7:
            w0[t] = 0.0 if rng.random() < 0.1 else (float(rng.random() * 1e3) if fractional else float(rng.integers(1, 10 ** 6)))
    glen = rng.integers(1000, 9000, size=T).astype(np.float64)
    return off, tax, hitlen, w0, glen


def definition(w0, off, tax, hitlen, glen=None, max_iter=1, tol=0.0, changes=None):
    """metalign_amd/multimap.py over arrays -> (extra float64[T], touched bool[T], iterations_run, last_change)."""
    w = [None if x != x else float(x) for x in w0]
    extra, touched, n, c = mmdef.iterate(w, [int(x) for x in off], [int(x) for x in tax], [int(x) for x in hitlen],
                                         None if glen is None else [float(x) for x in glen], max_iter, tol, changes)
    return np.array(extra, dtype=np.float64), np.array(touched, dtype=bool), n, c


def weights(w0, extra):
    """w_i = w0 + extra_i over the taxa with an entry (NaN elsewhere)."""
    return np.asarray(w0, dtype=np.float64) + np.asarray(extra, dtype=np.float64)


def trajectory(w0, off, tax, hitlen, glen, iters):
    """The definition's weights after each iteration in `iters` -> {i: float64[T]} (one run to max(iters), tol = 0)."""
    w0l = [None if x != x else float(x) for x in w0]
    o, t, h = [int(x) for x in off], [int(x) for x in tax], [int(x) for x in hitlen]
    gl = None if glen is None else [float(x) for x in glen]
    w, out = list(w0l), {}
    for i in range(1, max(iters) + 1):
        extra, touched = mmdef.step(w, o, t, h, gl)
        w = mmdef.new_weights(w0l, extra, touched)
        if i in iters:
            out[i] = np.array([NAN if x is None else x for x in w], dtype=np.float64)
    return out


def decimal_weights(w0, off, tax, hitlen, glen, iters, digits=50):
    """The definition in decimal arithmetic of `digits` digits -> {i: [w_i[t] as Decimal or None]} for i in iters."""
    ctx = decimal.Context(prec=digits)
    D = decimal.Decimal
    w0d = [None if x != x else D(float(x)) for x in w0]
    gl = None if glen is None else [D(float(x)) for x in glen]
    lists = [sorted({t for t in row if w0d[t] is not None}) for row in as_lists(off, tax)]
    hl = [D(int(x)) for x in hitlen]
    w, out = list(w0d), {}
    for i in range(1, max(iters) + 1):
        extra = [D(0)] * len(w0d)
        for taxa, h in zip(lists, hl):
            if not taxa:
                continue
            den = D(0)
            for t in taxa:
                den = ctx.add(den, w[t])
            if den == 0:
                continue
            for t in taxa:
                part = ctx.multiply(ctx.divide(w[t], den), h)
                if gl is not None:
                    part = ctx.divide(part, gl[t])
                extra[t] = ctx.add(extra[t], part)
        w = [None if a is None else ctx.add(a, e) for a, e in zip(w0d, extra)]
        if i in iters:
            out[i] = list(w)
    return out


def rel_dev(w, yard):
    """Largest relative deviation of float weights from decimal ones, over the taxa with an entry."""
    D = decimal.Decimal
    worst = D(0)
    for a, y in zip(w, yard):
        if y is None:
            continue
        d = abs(D(float(a)) - y)
        worst = max(worst, d / y if y != 0 else d)
    return float(worst)


def permuted(rng, off, tax, hitlen):
    """The same reads in another order: each read's block of mm_tax moves whole, its internal order stays."""
    rows = as_lists(off, tax)
    order = rng.permutation(len(rows))
    o2, t2 = csr([rows[i] for i in order])
    return o2, t2, np.asarray(hitlen, dtype=np.uint64)[order]


def records(rec_dtype, lists, hitlens):
    """Alignment records from which stage C makes the multimapped CSR `lists` (dense taxon = reference row; lists of >= 2 entries):
    a single-end read with n retained lines is a multimapped read of n taxa in file order, its hitlen the summed SEQ lengths (here:
    all on its first line).  A dummy read of two lines goes first (the first boundary is always Ambiguous, and the read behind an
    Ambiguous one loses its first line: one line is left, a unique read) and a dummy read last (the last read is never processed)."""
    n = sum(len(x) for x in lists) + 3
    recs = np.zeros(n, dtype=rec_dtype)
    recs["total"] = 100
    recs["matched"] = 100
    ref = np.zeros(n, dtype=np.uint32)
    new = np.zeros(n, dtype=np.uint32)
    ln = np.zeros(n, dtype=np.uint32)
    new[0] = new[-1] = 1
    k = 2
    for taxa, h in zip(lists, hitlens):
        assert len(taxa) >= 2 and 0 <= int(h) < (1 << 20)
        ref[k:k + len(taxa)] = taxa
        new[k] = 1
        ln[k] = int(h)
        k += len(taxa)
    recs["ref_new"] = ref | (new << np.uint32(31))
    recs["flag_len"] = ln << np.uint32(12)
    return recs
