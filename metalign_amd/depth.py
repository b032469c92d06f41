"""Per-base depth of coverage from stage C's alignments (--depth, --depth_windows): the definition, on the host.

Which lines count, where they lie and what an accession's length is are coverage.py's rules (its functions are used, not
restated).  On top of them:

  Depth.  depth[p] (0 <= p < L) of accession a = the number of counting, placed lines whose clipped block
      [pos0, min(pos0 + span, L)) contains p.  The bases under a D or N gap count.  Unplaced lines are counted as coverage does.
      Computed by sorting the intervals' end points and sweeping them: no per-base array, so 2^31-base accessions are fine.
  Histogram.  c[p] = min(depth[p], CAP), CAP = 4095; H_a[d] = the positions of a with c = d (only non-empty bins are kept), so the
      bins of H_a sum to L.  A genome's H is the sum over ALL its accessions; one that was never hit gives {0: L}.
  Statistics (stats), from H alone, exact (integers and Fractions), printed with %d / %.6f: mean_depth = sum(c H) / L;
      median_depth = the bin that holds ascending rank (L - 1) // 2; trimmed_mean_depth = the mean of ranks t .. L - 1 - t with
      t = L * 5 // 100 (CoverM's trimmed_mean at its default 5-95 %); depth_variance = the population variance of c; max_depth =
      the highest non-empty bin (CAP: "CAP or more"); bases_ge_1 / 5 / 10 / 30.
  Windows (window = W >= 1).  Window j of a is [j W, min((j + 1) W, L)); depth_sum = the sum of depth[p] over it, NOT clamped,
      covered = the positions with depth > 0.  Only windows with depth_sum > 0 are kept.

Everything is integer and independent of order, so the device (mg_depth.hip) is held to this exactly.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np

from .coverage import FLAG_MASK, _text, counts, lengths_of, matched_total, placement, retained_fields

CAP = 4095
HEADER = ('#kind\tid\ttaxid\tlength\tmean_depth\tmedian_depth\ttrimmed_mean_depth\tdepth_variance\tmax_depth\tbases_ge_1\tbases_ge_5'
          '\tbases_ge_10\tbases_ge_30\n')
WINDOWS_HEADER = '#accession\tstart\tend\tmean_depth\tcovered_bases\n'

# lengths {accession: L}; per {accession: [alignments, {clamped depth: positions}]} (accessions with a placed line); unplaced;
# window = W (0: none asked for); windows {accession: [(j, depth_sum, covered)] ascending, depth_sum > 0}
Depth = namedtuple('Depth', 'lengths per unplaced window windows')
Stats = namedtuple('Stats', 'length mean median trimmed variance max ge1 ge5 ge10 ge30')


def _segments(intervals):
    """Half-open intervals [(begin, end)] -> [(begin, end, depth)], depth >= 1, ascending and disjoint: the sweep."""
    events = {}
    for b, e in intervals:
        events[b] = events.get(b, 0) + 1
        events[e] = events.get(e, 0) - 1
    out, cur, last = [], 0, None
    for p in sorted(events):
        if cur > 0:
            out.append((last, p, cur))
        cur += events[p]
        last = p
    assert cur == 0
    return out


def histogram(segments, L):
    """The sweep's segments -> {clamped depth: positions}, bins summing to L."""
    H, covered = {}, 0
    for b, e, d in segments:
        c = min(d, CAP)
        H[c] = H.get(c, 0) + (e - b)
        covered += e - b
    if L - covered:
        H[0] = L - covered
    return H


def windows_of(segments, W):
    """The sweep's segments -> [(j, depth_sum, covered)] of the windows of width W they touch, ascending."""
    js, sums, covs = [], [], []
    for b, e, d in segments:
        j = np.arange(b // W, (e - 1) // W + 1, dtype=np.int64)
        width = np.minimum(e, (j + 1) * W) - np.maximum(b, j * W)
        js.append(j)
        sums.append(width * d)
        covs.append(width)
    if not js:
        return []
    j, s, c = np.concatenate(js), np.concatenate(sums), np.concatenate(covs)
    first = np.flatnonzero(np.concatenate(([True], j[1:] != j[:-1])))  # (segments ascend, so equal windows are neighbours)
    return list(zip(j[first].tolist(), np.add.reduceat(s, first).tolist(), np.add.reduceat(c, first).tolist()))


def accumulate(placed, lengths, window=0):
    """[(accession, pos0, span)] of COUNTING lines -> (per, unplaced, windows) of Depth."""
    intervals, unplaced = {}, 0
    for acc, pos0, span in placed:
        L = lengths[acc]
        if span == 0 or pos0 >= L:
            unplaced += 1
            continue
        intervals.setdefault(acc, []).append((pos0, min(pos0 + span, L)))
    per, windows = {}, {}
    for acc, iv in intervals.items():
        seg = _segments(iv)
        per[acc] = [len(iv), histogram(seg, lengths[acc])]
        if window:
            windows[acc] = windows_of(seg, window)
    return per, unplaced, windows


def depth(lines, acc2info, pct_id, window=0):
    """SAM lines (str or bytes; the header among them) -> Depth."""
    header, placed, leading = [], [], True
    for line in lines:
        if leading:
            if _text(line).startswith('@'):
                header.append(line)
                continue
            leading = False
        f = retained_fields(line)
        if f is None:
            continue
        acc2info[f[2]]  # KeyError for an RNAME db_info does not know, as coverage
        matched, total = matched_total(f)
        if not counts(int(f[1]), matched, total, pct_id):
            continue
        placed.append((f[2],) + placement(f))
    lengths = lengths_of(header, acc2info)
    per, unplaced, windows = accumulate(placed, lengths, window)
    return Depth(lengths, per, unplaced, window, windows)


def depth_of_records(recs, places, accessions, lengths, pct_id, window=0):
    """The same from (record, place) pairs, with coverage.coverage_of_records' conventions."""
    placed, no_row = [], 0
    for r, (pos0, span) in zip(recs, places):
        if not counts(int(r['flag_len']) & FLAG_MASK, int(r['matched']), int(r['total']), pct_id):
            continue
        row = int(r['ref_new']) & 0x7FFFFFFF
        if row >= len(accessions):  # (no such accession: the device counts the record as unplaced)
            no_row += 1
            continue
        placed.append((accessions[row], int(pos0), int(span)))
    per, unplaced, windows = accumulate(placed, lengths, window)
    return Depth(lengths, per, unplaced + no_row, window, windows)


def _rank_sum(bins, lo, hi):
    """The sum of c over ascending ranks lo .. hi (inclusive) of the sorted bins [(c, count)]."""
    total, at = 0, 0
    for c, n in bins:
        b, e = max(at, lo), min(at + n, hi + 1)
        if e > b:
            total += c * (e - b)
        at += n
    return total


def stats(H):
    """{clamped depth: positions} -> Stats, exact; a histogram without positions gives zeros."""
    bins = sorted((c, n) for c, n in H.items() if n)
    L = sum(n for _, n in bins)
    if L == 0:
        return Stats(0, Fraction(0), 0, Fraction(0), Fraction(0), 0, 0, 0, 0, 0)
    s1 = sum(c * n for c, n in bins)
    s2 = sum(c * c * n for c, n in bins)
    rank, at, median = (L - 1) // 2, 0, 0
    for c, n in bins:
        if at + n > rank:
            median = c
            break
        at += n
    t = L * 5 // 100
    trimmed = Fraction(_rank_sum(bins, t, L - 1 - t), L - 2 * t)
    ge = [sum(n for c, n in bins if c >= k) for k in (1, 5, 10, 30)]
    return Stats(L, Fraction(s1, L), median, trimmed, Fraction(s2, L) - Fraction(s1, L) ** 2, bins[-1][0], *ge)


def rows(dep, acc2info, taxid2info):
    """-> [(kind, id, taxid, length, H)]: the accessions and taxids of coverage.rows, in its order; a genome's H sums ALL its
    accessions' (one never hit: {0: L})."""
    out, by_tax = [], {}
    for acc, info in acc2info.items():
        g = by_tax.setdefault(info[1], [0, 0, {}])
        L = dep.lengths[acc]
        g[0] += L
        st = dep.per.get(acc)
        H = st[1] if st is not None else ({0: L} if L else {})
        for c, n in H.items():
            g[2][c] = g[2].get(c, 0) + n
        if st is None:
            continue
        out.append(('S', acc, info[1], L, st[1]))
        g[1] += st[0]
    for taxid in taxid2info:
        g = by_tax.get(taxid)
        if g is not None and g[1] >= 1:
            out.append(('G', taxid, taxid, g[0], g[2]))
    return out


def format_row(row):
    kind, ident, taxid, length, H = row
    s = stats(H)
    return '%s\t%s\t%s\t%d\t%.6f\t%d\t%.6f\t%.6f\t%d\t%d\t%d\t%d\t%d\n' % (
        kind, ident, taxid, length, float(s.mean), s.median, float(s.trimmed), float(s.variance), s.max, s.ge1, s.ge5, s.ge10, s.ge30)


def format_block(block_rows, unplaced, source=None):
    """One input file's block: `#file\\t<source>` (several input files only), its rows, `#unplaced\\t<n>`."""
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_row(r) for r in block_rows) + '#unplaced\t%d\n' % unplaced


def write_depth(path, block_rows=None, unplaced=0, source=None, append=False):
    """TSV: the column header (a new file only), then — unless block_rows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER)
        if block_rows is not None:
            out.write(format_block(block_rows, unplaced, source))


def window_rows(dep, acc2info):
    """-> [(accession, start, end, depth_sum, covered)]: the kept windows, accessions in db_info order, windows ascending."""
    out, W = [], dep.window
    for acc in acc2info:
        L = dep.lengths[acc]
        for j, dsum, cov in dep.windows.get(acc, ()):
            out.append((acc, j * W, min((j + 1) * W, L), dsum, cov))
    return out


def format_window_row(row):
    acc, start, end, dsum, cov = row
    return '%s\t%d\t%d\t%.6f\t%d\n' % (acc, start, end, float(Fraction(dsum, end - start)), cov)


def format_window_block(wrows, source=None):
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_window_row(r) for r in wrows)


def write_windows(path, wrows=None, source=None, append=False):
    """TSV: the column header (a new file only), then — unless wrows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(WINDOWS_HEADER)
        if wrows is not None:
            out.write(format_window_block(wrows, source))
