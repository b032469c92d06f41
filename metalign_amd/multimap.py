"""--multimap_iterations: multimapped-read reassignment run as a fixed-point iteration.  This file is the definition.

resolve_multi_prop (scripts/map_and_profile.py:269-312) shares each multimapped read once among its taxa, in proportion to their
uniquely mapped bases.  That is the first step of the expectation-maximisation GRAMMy, Pathoscope and Bracken's re-estimation run
to a fixed point: the shares of step i are taken in proportion to the weights step i-1 gave.  Plain Python floats, no numpy in
the arithmetic; the host routine (mg_multimapped_shares_iter) equals this bit for bit, the device path
(mg_profile_mm_iterate_dev) up to the order of its additions.

Inputs, over dense taxon ids t = 0 .. T-1 (the ids of the multimapped CSR):
  w0[t]         the taxon's bases after the read cutoff; None or NaN: the taxon has no entry in taxids2abs
  mm_offsets, mm_tax, mm_hitlen   the multimapped CSR: read r has the taxa mm_tax[mm_offsets[r]:mm_offsets[r+1]] and mm_hitlen[r] bases
  genome_len[t] or None           --length_normalize
  max_iter >= 1, tol >= 0

Iteration i = 1, 2, ..., with w_0 = w0:
  per read, in file order: its DISTINCT taxa that have an entry, in ascending order of their dense id (the order of the library's
    one step, mg_multimapped_shares, and of resolve_multi_prop_csr: this is what makes one iteration today's result bit for bit —
    with the whole-number weights of the first step the order of a read's own taxa cannot show, later it can);
    den = the sum of their w_{i-1}, added left to right; the read is skipped when it has no such taxon or den == 0.0 — decided
    anew in every iteration (within one run the answer never changes: a weight of exactly 0.0 cannot grow, its share is 0 / den = 0
    and w_i = w0 + 0, so a read whose weights are all 0 stays out of every iteration);
    part = (w_{i-1}[t] / den) * hitlen, then / genome_len[t] if given; extra_i[t] += part, read after read
  w_i[t] = w0[t] + extra_i[t] for the taxa a read touched, w0[t] for the others
  change_i = max over the taxa with an entry of |w_i[t] - w_{i-1}[t]| / w_i[t]   (a taxon with w_i[t] == 0 counts 0)
  stop after iteration i when i == max_iter, or when tol > 0 and change_i <= tol

Hand example: taxa A, B, C with w0 = (300, 100, 100); reads {A,B}, {A,B}, {B,C}, {B,C}, 100 bases each.
  after 1 iteration  (450, 250, 200)
  after 2            (300 + 900/7, 100 + 500/7 + 1000/9, 100 + 800/9) ~ (428.571429, 282.539683, 188.888889)
  the total stays 900 (without genome lengths every read hands out exactly its bases).
"""


def _has_entry(w):
    return w is not None and w == w


def step(w_prev, mm_offsets, mm_tax, mm_hitlen, genome_len=None):
    """One pass over the reads with the weights w_prev -> (extra, touched)."""
    T = len(w_prev)
    extra = [0.0] * T
    touched = [False] * T
    for r in range(len(mm_hitlen)):
        taxa = sorted({int(t) for t in mm_tax[int(mm_offsets[r]):int(mm_offsets[r + 1])] if _has_entry(w_prev[int(t)])})
        if not taxa:
            continue
        den = 0.0
        for t in taxa:
            den += w_prev[t]
        if den == 0.0:
            continue
        hitlen = float(int(mm_hitlen[r]))
        for t in taxa:
            part = (w_prev[t] / den) * hitlen
            if genome_len is not None:
                part = part / float(genome_len[t])
            extra[t] += part
            touched[t] = True
    return extra, touched


def new_weights(w0, extra, touched):
    return [(w0[t] + extra[t] if touched[t] else w0[t]) if _has_entry(w0[t]) else None for t in range(len(w0))]


def change(w_new, w_old):
    c = 0.0
    for a, b in zip(w_new, w_old):
        if a is None or a == 0.0:
            continue
        d = abs(a - b) / a
        if d > c:
            c = d
    return c


def iterate(w0, mm_offsets, mm_tax, mm_hitlen, genome_len=None, max_iter=1, tol=0.0, changes=None):
    """-> (extra, touched, iterations_run, last_change): what the last iteration adds to w0, per dense taxon id.
    changes: a list that receives change_1, change_2, ..."""
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    if not tol >= 0:
        raise ValueError('tol must not be negative')
    w0 = [float(w) if _has_entry(w) else None for w in w0]
    w = list(w0)
    i = 0
    while True:
        i += 1
        extra, touched = step(w, mm_offsets, mm_tax, mm_hitlen, genome_len)
        w_new = new_weights(w0, extra, touched)
        c = change(w_new, w)
        if changes is not None:
            changes.append(c)
        w = w_new
        if i == max_iter or (tol > 0 and c <= tol):
            return extra, touched, i, c


def resolve(taxids2abs, taxids, mm_offsets, mm_tax, mm_hitlen, genome_len=None, max_iter=1, tol=0.0):
    """The iteration over a taxids2abs dict (taxid -> [reads, bases]); taxids[t] names dense id t.  taxids2abs[t][1] becomes w_i[t].
    -> (iterations_run, last_change)."""
    w0 = [float(taxids2abs[t][1]) if t in taxids2abs else None for t in taxids]
    extra, touched, n, c = iterate(w0, mm_offsets, mm_tax, mm_hitlen, genome_len, max_iter, tol)
    for i, t in enumerate(taxids):
        if touched[i]:
            taxids2abs[t][1] = w0[i] + extra[i]
    return n, c
