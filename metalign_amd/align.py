"""Short reads aligned to the reference FASTA by seed and extend (--aligner device): the definition, on the host.

This is NOT a port of minimap2 and claims no parity with it: it is a small aligner of its own, defined here so that the device
(mg_align.hip; the per-position rules are in mg_align_core.h and mg_align_gap_core.h) can be held to it exactly.  Without
--align_band it is UNGAPPED: a read whose only good alignment needs an insertion or deletion aligns in part or not at all.  With
--align_band B > 0 a candidate whose ungapped segment is shorter than its read is refined by a banded local alignment with affine
gaps (extend_gapped), which finds insertions and deletions of up to B bases.  It keeps no names and gives no MAPQ.  Without
--align_pairs it knows no pairs: every read counts as its own read, each primary record carries the new-read bit, whatever the
read's name — two reads of one name (the mates of a pair in one file) are two reads.  With --align_pairs interleaved reads 2i and
2i + 1 are the mates of pair i, BY POSITION (no name is compared): see "Pairs" below.

  Codes.  refseq.codes_of: A a 0, C c 1, G g 2, T t 3, every other byte 4.  The complement of a code c < 4 is 3 - c, of 4 it is 4.
  k-mers.  k odd, 11 .. 31.  A k-mer with a code 4 has no key.  Otherwise f = its 2k-bit value (first base most significant), r =
      that of its reverse complement; the strand bit is 0 if f < r else 1 (never equal: k is odd); the key is fmix64(min(f, r)),
      a bijection, so equal keys mean equal canonical k-mers.
  Minimizers.  n bases have m = max(0, n - k + 1) positions; the windows are [s, min(s + w, m)) for s = 0 .. max(0, m - w) (none when
      m = 0); a window's minimizer is its keyed position of the smallest key, the leftmost among equals; the minimizers of a
      sequence are the distinct positions some window chose.
  Index.  (key, a, p, s) for every minimizer of every loaded accession row a.  occ(key) = its entries.
  Candidates.  Only a read of k <= L <= 1024 bases has any.  Every minimizer (key, i, s_r) of the read with 1 <= occ(key) <= max_occ
      meets every entry (key, a, p, s_g): strand 0 with diagonal d = p - i where s_r == s_g, else strand 1 with d = p - (L - k - i).
      The candidates are the DISTINCT (a, strand, d).
  Extension.  extend(): the best segment of the scan along the diagonal, the first to reach the highest score.
  Gapped extension.  Off at band 0.  Otherwise an accepted candidate (ungapped score >= min_score) with e - b < L is REFINED: it
      takes the result of extend_gapped() on its diagonal in place of the scan's.  The cells are (i, j), 0 <= i < L, 0 <= j < n,
      |j - i - d| <= B; s(i, j) = +1 if o[i] < 4 and o[i] == g[j] else -P; with O = gap_open, E = gap_extend (a gap of g bases
      costs O + g E):
          X(i, j) = (H(i-1, j-1) if that cell exists else 0) + s(i, j)
          I(i, j) = max(H(i-1, j) - O - E, I(i-1, j) - E) if cell (i-1, j) exists, else none
          D(i, j) = max(H(i, j-1) - O - E, D(i, j-1) - E) if cell (i, j-1) exists, else none
          H(i, j) = max(0, X, I, D)
      The best cell has the largest H, then the smallest i, then the smallest j.  The walk back from it is decided by values
      alone: in state H, H == X emits an M column and goes to (i-1, j-1), stopping first where that cell does not exist or its H
      is 0; else H == I switches to state I, else to state D.  State I emits an I column and goes to (i-1, j), in state H if
      I(i, j) == H(i-1, j) - O - E, else in state I; state D the same along j.  Diagonal before insertion before deletion, open
      before extend.  The band holds the candidate's own diagonal, so the refined score is never below the ungapped one.
  Selection.  select(): by (score descending, a, pos0, strand, d); no two kept alignments of one a and strand overlap on the
      reference ([pos0, pos0 + reference span)); secondaries need sec_pct % of the best score; at most 1 + max_secondary are kept.
      Two candidates either side of one indel refine to overlapping alignments and collapse to one.
  Records.  records(): what the device leaves in its batch.  A record's matched = its M columns and its total = every CIGAR
      operation's length, clips included, as stage C's tokenisers count a SAM line: L without gaps, L + the D columns with them.  sam_lines(): the same alignments as SAM text.
  Pairs (PairParams: interleaved, max_insert I, rescue R).  The place of an alignment x of a read of L bases is [u, v): u = pos0 - b,
      v = pos0 + span + (L - e), the whole oriented read, clips included (ungapped: u = d, v = d + L).
      concordant(): x of mate 1 and y of mate 2 on one accession and on different strands, and with f the strand-0 and r the
      strand-1 one: u(f) <= u(r), v(f) <= v(r), v(r) - u(f) <= I.
      Rescue (rescue_pair), after the ungapped extension and before the refinement, judged on the accepted sets A1, A2 as they
      were BEFORE any rescue: the anchors of mate m are the first R of A_m by order_key.  An anchor (a, s, d) of a mate of L
      bases, whose partner has k <= L' <= 1024 bases, seeks the partner on strand 1 - s of a over the diagonals rescue_window():
      s = 0: [d + max(0, L - L'), d + I - L'], s = 1: [d + L - I, d + min(0, L - L')], clipped to [1 - L', n - 1]; an empty
      range is no task, and neither is one where the partner's set holds a candidate (a, 1 - s, d'') with lo - B <= d'' <= hi + B
      (B: the band).  Otherwise extend() runs on every d' of the window; the best score wins, the smallest d' among equals, and
      joins the partner's accepted set if it reaches min_score (a set by (a, strand, d): found twice, added once).  With a band
      every accepted candidate with e - b < L is then refined, seeded or rescued.
      Selection (select_pair): C_m = pair_list(): the accepted set of mate m by order_key under the overlap rule, its first 16
      (select() is C_m filtered by sec_pct and cut at 1 + max_secondary).  The best concordant pair has the highest sum of scores,
      then the smallest place of x in C1, then of y in C2; x and y are the primaries, a secondary of a mate is another entry of
      its list whose best concordant partner gives 100 (x.score + y.score) >= sec_pct * best, at most max_secondary, and every
      record carries FLAG 1 + 2.  Without a concordant pair each mate is selected alone (select()) and carries FLAG 1, and 8
      where the partner has no record.  Always 64 / 128 for mate 1 / 2, 16 for the own strand, 32 where the partner's primary
      is on strand 1, 256 on secondaries.  The pair's records are mate 1's, then mate 2's; the new-read bit is on the first of
      them only; each mate's primary carries its own len(SEQ) and pile.  RNEXT, PNEXT and TLEN are not given.
"""
import re
from collections import namedtuple

import numpy as np

from . import refseq

K, W, MAX_OCC, MIN_SCORE, MISMATCH, MAX_SECONDARY, SEC_PCT = 15, 5, 64, 30, 4, 5, 80
MAX_READ = 1024
M64 = (1 << 64) - 1

# (the order of the fields of mg_align_params, include/metalign_hip.h)
Params = namedtuple('Params', 'k w max_occ min_score mismatch max_secondary sec_pct')
# one alignment of a read: [b, e) of the oriented read o on accession row a at pos0 = d + b
Aln = namedtuple('Aln', 'a strand d score b e nm')
Stats = namedtuple('Stats', 'reads aligned candidates accepted records')
# (the order of the fields of mg_align_gap) band 0: no gapped extension; a gap of g bases costs gap_open + g * gap_extend
GapParams = namedtuple('GapParams', 'band gap_open gap_extend')
BAND, GAP_OPEN, GAP_EXTEND, MAX_BAND = 0, 6, 1, 31
# a refined alignment: what Aln has (d: the candidate's diagonal), [pos0, pos0 + span) on the reference, one of M I D per column
GapAln = namedtuple('GapAln', 'a strand d score b e nm pos0 span ops')
GAP_CODE = 5  # (variants.GAP: a reference base under a deletion, in the pile)
# (the order of the fields of mg_align_pairs) interleaved 0: no pairs; max_insert: the largest outer distance of a proper pair;
# rescue: the anchors per mate that may rescue, 0: none
PairParams = namedtuple('PairParams', 'interleaved max_insert rescue')
MAX_INSERT, RESCUE, MAX_INSERT_LIMIT, MAX_RESCUE, PAIR_LIST = 1000, 2, 8192, 8, 16
PairStats = namedtuple('PairStats', 'refined rescued proper')


def params(k=K, w=W, max_occ=MAX_OCC, min_score=MIN_SCORE, mismatch=MISMATCH, max_secondary=MAX_SECONDARY, sec_pct=SEC_PCT):
    """-> Params; ValueError names the first value out of its range."""
    p = Params(int(k), int(w), int(max_occ), int(min_score), int(mismatch), int(max_secondary), int(sec_pct))
    if p.k < 11 or p.k > 31 or p.k % 2 == 0:
        raise ValueError('--align_k must be odd and within 11 to 31.')
    if p.w < 1 or p.w > 32:
        raise ValueError('--align_w must be within 1 to 32.')
    if p.max_occ < 1 or p.max_occ > 65535:
        raise ValueError('--align_max_occ must be within 1 to 65535.')
    if p.min_score < 1 or p.min_score > MAX_READ:
        raise ValueError('--align_min_score must be within 1 to %d.' % MAX_READ)
    if p.mismatch < 1 or p.mismatch > 64:
        raise ValueError('--align_mismatch must be within 1 to 64.')
    if p.max_secondary < 0 or p.max_secondary > 15:
        raise ValueError('--align_secondary must be within 0 to 15.')
    if p.sec_pct < 0 or p.sec_pct > 100:
        raise ValueError('--align_secondary_pct must be within 0 to 100.')
    return p


def gap_params(band=BAND, gap_open=GAP_OPEN, gap_extend=GAP_EXTEND):
    """-> GapParams; ValueError names the first value out of its range."""
    g = GapParams(int(band), int(gap_open), int(gap_extend))
    if g.band < 0 or g.band > MAX_BAND:
        raise ValueError('--align_band must be within 0 to %d.' % MAX_BAND)
    if g.gap_open < 0 or g.gap_open > 64:
        raise ValueError('--align_gap_open must be within 0 to 64.')
    if g.gap_extend < 1 or g.gap_extend > 64:
        raise ValueError('--align_gap_extend must be within 1 to 64.')
    return g


def pair_params(interleaved=0, max_insert=MAX_INSERT, rescue=RESCUE):
    """-> PairParams; ValueError names the first value out of its range."""
    if interleaved in ('none', 'interleaved'):
        interleaved = int(interleaved == 'interleaved')
    pp = PairParams(int(interleaved), int(max_insert), int(rescue))
    if pp.interleaved not in (0, 1):
        raise ValueError('--align_pairs must be "none" or "interleaved".')
    if pp.max_insert < 1 or pp.max_insert > MAX_INSERT_LIMIT:
        raise ValueError('--align_max_insert must be within 1 to %d.' % MAX_INSERT_LIMIT)
    if pp.rescue < 0 or pp.rescue > MAX_RESCUE:
        raise ValueError('--align_rescue must be within 0 to %d.' % MAX_RESCUE)
    return pp


def fmix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def revcomp_codes(codes):
    return bytes(3 - c if c < 4 else 4 for c in reversed(codes))


def kmer_keys(codes, k):
    """-> [(key, strand bit) or None] for the max(0, n - k + 1) positions."""
    n, mask, top = len(codes), (1 << (2 * k)) - 1, 2 * (k - 1)
    out, f, r, valid = [], 0, 0, 0
    for i, c in enumerate(codes):
        if c < 4:
            f = ((f << 2) | c) & mask
            r = (r >> 2) | ((3 - c) << top)
            valid += 1
        else:
            f = r = valid = 0
        if i >= k - 1:
            out.append((fmix64(min(f, r)), 0 if f < r else 1) if valid >= k else None)
    assert len(out) == max(0, n - k + 1)
    return out


def minimizers(codes, k, w):
    """-> [(key, position, strand bit)], by position."""
    keys = kmer_keys(codes, k)
    m, chosen = len(keys), set()
    if m == 0:
        return []
    for s in range(0, max(0, m - w) + 1):
        best = None
        for q in range(s, min(s + w, m)):
            if keys[q] is not None and (best is None or keys[q][0] < keys[best][0]):
                best = q
        if best is not None:
            chosen.add(best)
    return [(keys[q][0], q, keys[q][1]) for q in sorted(chosen)]


def index_entries(ref, k, w):
    """ref: refseq.RefSeq (codes {row: bytes of codes}, loaded) -> the sorted list of (key, a, p, s)."""
    out = []
    for a, is_loaded in enumerate(ref.loaded):
        if is_loaded:
            out.extend((key, a, p, s) for key, p, s in minimizers(ref.codes[a], k, w))
    return sorted(out)


def build_index(ref, k, w):
    """-> {key: [(a, p, s)]}."""
    index = {}
    for key, a, p, s in index_entries(ref, k, w):
        index.setdefault(key, []).append((a, p, s))
    return index


def candidates(codes, index, p):
    """The read's codes -> the set of (a, strand, d)."""
    L = len(codes)
    out = set()
    if L < p.k or L > MAX_READ:
        return out
    for key, i, s_r in minimizers(codes, p.k, p.w):
        entries = index.get(key, ())
        if 1 <= len(entries) <= p.max_occ:
            for a, pos, s_g in entries:
                out.add((a, 0, pos - i) if s_r == s_g else (a, 1, pos - (L - p.k - i)))
    return out


def scan(cols, P):
    """The scan over one column pattern: cols[j] is None (outside), True (adds 1) or False (subtracts P) -> (score, b, e)."""
    cur, start, best = 0, 0, (0, 0, 0)
    for j, c in enumerate(cols):
        if c is None:
            cur, start = 0, j + 1
            continue
        cur += 1 if c else -P
        if cur <= 0:
            cur, start = 0, j + 1
        elif cur > best[0]:
            best = (cur, start, j + 1)
    return best


def columns(o, ref_codes, d):
    n = len(ref_codes)
    return [None if d + j < 0 or d + j >= n else (c < 4 and c == ref_codes[d + j]) for j, c in enumerate(o)]


def extend(o, ref_codes, d, P):
    """-> (score, b, e, nm) of the oriented read o on the diagonal d of one accession's codes."""
    cols = columns(o, ref_codes, d)
    score, b, e = scan(cols, P)
    return score, b, e, sum(1 for c in cols[b:e] if not c)


def gap_cells(o, ref_codes, d, P, gp):
    """The banded table: rows[i][t] = (H, I, D) of cell (i, j = i + d + t - B), I or D None where it has none, or None where the
    cell does not exist."""
    B, O, E = gp
    n, rows = len(ref_codes), []
    for i, c in enumerate(o):
        row, prev = [None] * (2 * B + 1), rows[-1] if rows else None
        for t in range(2 * B + 1):
            j = i + d + t - B
            if j < 0 or j >= n:
                continue
            diag = prev[t] if prev is not None else None  # (i - 1, j - 1)
            up = prev[t + 1] if prev is not None and t < 2 * B else None  # (i - 1, j)
            left = row[t - 1] if t > 0 else None  # (i, j - 1)
            X = (diag[0] if diag is not None else 0) + (1 if c < 4 and c == ref_codes[j] else -P)
            ins = None if up is None else max(up[0] - O - E, up[1] - E if up[1] is not None else up[0] - O - E)
            dele = None if left is None else max(left[0] - O - E, left[2] - E if left[2] is not None else left[0] - O - E)
            row[t] = (max(0, X, ins if ins is not None else 0, dele if dele is not None else 0), ins, dele)
        rows.append(row)
    return rows


def extend_gapped(o, ref_codes, d, P, gp):
    """-> (score, b, e, nm, pos0, span, ops) of the banded local alignment with affine gaps of the oriented read o around the
    diagonal d of one accession's codes; ops: one of M I D per column.  Score 0: (0, 0, 0, 0, 0, 0, '')."""
    B, O, E = gp
    rows = gap_cells(o, ref_codes, d, P, gp)
    best = (0, 0, 0)
    for i, row in enumerate(rows):
        for t, cell in enumerate(row):
            if cell is not None and cell[0] > best[0]:
                best = (cell[0], i, t)
    score, i, t = best
    if score == 0:
        return 0, 0, 0, 0, 0, 0, ''

    def at(i, t):
        return rows[i][t] if 0 <= i and 0 <= t <= 2 * B else None

    e, j_end, ops, nm, state = i + 1, i + d + t - B, [], 0, 'H'
    while True:
        H, ins, dele = rows[i][t]
        if state == 'H':
            diag = at(i - 1, t)
            if H == (diag[0] if diag is not None else 0) + (1 if o[i] < 4 and o[i] == ref_codes[i + d + t - B] else -P):
                ops.append('M')
                nm += 0 if o[i] < 4 and o[i] == ref_codes[i + d + t - B] else 1
                if diag is None or diag[0] == 0:
                    break
                i -= 1
            elif ins is not None and H == ins:
                state = 'I'
            else:
                assert dele is not None and H == dele
                state = 'D'
        elif state == 'I':
            ops.append('I')
            nm += 1
            state = 'H' if ins == at(i - 1, t + 1)[0] - O - E else 'I'
            i, t = i - 1, t + 1
        else:
            ops.append('D')
            nm += 1
            state = 'H' if dele == at(i, t - 1)[0] - O - E else 'D'
            t -= 1
    pos0 = i + d + t - B
    return score, i, e, nm, pos0, j_end - pos0 + 1, ''.join(reversed(ops))


def pos0_of(al):
    return al.pos0 if isinstance(al, GapAln) else al.d + al.b


def span_of(al):
    """The reference span."""
    return al.span if isinstance(al, GapAln) else al.e - al.b


def ops_of(al):
    return al.ops if isinstance(al, GapAln) else 'M' * (al.e - al.b)


def order_key(al):
    return (-al.score, al.a, pos0_of(al), al.strand, al.d)


def select(accepted, p):
    """Accepted alignments (Aln) of one read -> the kept ones, the primary first."""
    kept = []
    for al in sorted(accepted, key=order_key):
        pos0, span = pos0_of(al), span_of(al)
        if any(x.a == al.a and x.strand == al.strand and pos0_of(x) < pos0 + span and pos0 < pos0_of(x) + span_of(x) for x in kept):
            continue
        if kept and al.score * 100 < kept[0].score * p.sec_pct:
            continue
        kept.append(al)
        if len(kept) == 1 + p.max_secondary:
            break
    return kept


def align_read_gapped(seq, index, ref, p, gp):
    """One read's bytes -> (kept alignments: Aln, or GapAln where refined; distinct, accepted and refined candidates)."""
    codes = refseq.codes_of(seq)
    cands = candidates(codes, index, p)
    if not cands:
        return [], 0, 0, 0
    rc = revcomp_codes(codes)
    accepted, refined = [], 0
    for a, strand, d in cands:
        o = rc if strand else codes
        score, b, e, nm = extend(o, ref.codes[a], d, p.mismatch)
        if score < p.min_score:
            continue
        if gp.band > 0 and e - b < len(o):
            g = extend_gapped(o, ref.codes[a], d, p.mismatch, gp)
            assert g[0] >= score, (g, score)  # (the band holds the diagonal)
            accepted.append(GapAln(a, strand, d, *g))
            refined += 1
        else:
            accepted.append(Aln(a, strand, d, score, b, e, nm))
    return select(accepted, p), len(cands), len(accepted), refined


def align_read(seq, index, ref, p):
    """One read's bytes -> (kept alignments, distinct candidates, accepted candidates)."""
    return align_read_gapped(seq, index, ref, p, GapParams(0, GAP_OPEN, GAP_EXTEND))[:3]


def align_reads_gapped(seqs, ref, p, gp, index=None):
    """-> ([kept alignments per read], Stats, refined candidates)."""
    if index is None:
        index = build_index(ref, p.k, p.w)
    out, ncand, nacc, nref = [], 0, 0, 0
    for seq in seqs:
        kept, c, a, r = align_read_gapped(seq, index, ref, p, gp)
        out.append(kept)
        ncand += c
        nacc += a
        nref += r
    return out, Stats(len(seqs), sum(1 for x in out if x), ncand, nacc, sum(len(x) for x in out)), nref


def align_reads(seqs, ref, p, index=None):
    """-> ([kept alignments per read], Stats)."""
    return align_reads_gapped(seqs, ref, p, GapParams(0, GAP_OPEN, GAP_EXTEND), index)[:2]


def place_of(al, L):
    """-> (u, v): where the whole oriented read of L bases lies on the reference, clips included."""
    pos0 = pos0_of(al)
    return pos0 - al.b, pos0 + span_of(al) + (L - al.e)


def concordant(x, Lx, y, Ly, I):
    """x of one mate (Lx bases) and y of the other: a proper pair within the outer distance I?"""
    if x.a != y.a or x.strand == y.strand:
        return False
    (uf, vf), (ur, vr) = (place_of(x, Lx), place_of(y, Ly)) if x.strand == 0 else (place_of(y, Ly), place_of(x, Lx))
    return uf <= ur and vf <= vr and vr - uf <= I


def rescue_window(strand, d, L, Lp, n, I):
    """An anchor on (strand, d) of a mate of L bases, its partner of Lp bases, an accession of n bases -> (lo, hi): the diagonals
    of strand 1 - strand on which the partner is sought, or None for an empty range."""
    lo, hi = (d + max(0, L - Lp), d + I - Lp) if strand == 0 else (d + L - I, d + min(0, L - Lp))
    lo, hi = max(lo, 1 - Lp), min(hi, n - 1)
    return (lo, hi) if lo <= hi else None


def window_scores(o, ref_codes, lo, hi, P):
    """extend(o, ref_codes, d, P)[0] for every d of [lo, hi], all diagonals at once (tests hold it to extend())."""
    n, Lp, W = len(ref_codes), len(o), hi - lo + 1
    g = np.full(W + Lp - 1, 255, dtype=np.uint8)
    s, e = max(lo, 0), min(hi + Lp, n)
    if s < e:
        g[s - lo:e - lo] = np.frombuffer(bytes(ref_codes), dtype=np.uint8)[s:e]
    cur, best = np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.int32)
    for j, c in enumerate(o):
        col = g[j:j + W]
        step = np.where(col == c, 1, -P).astype(np.int32) if c < 4 else np.full(W, -P, dtype=np.int32)
        cur = np.where(col != 255, np.maximum(cur + step, 0), 0).astype(np.int32)
        np.maximum(best, cur, out=best)
    return best


def rescue_pair(codes, accepted, ref, p, gp, pp):
    """codes: the two mates' codes; accepted: their accepted sets before any rescue (lists of Aln) -> ([the alignments rescue
    adds to mate 1's set, to mate 2's], the tasks)."""
    added, tasks = [{}, {}], 0
    for m in (0, 1):
        L, Lp = len(codes[m]), len(codes[1 - m])
        if Lp < p.k or Lp > MAX_READ:
            continue
        for x in sorted(accepted[m], key=order_key)[:pp.rescue]:
            win = rescue_window(x.strand, x.d, L, Lp, len(ref.codes[x.a]), pp.max_insert)
            if win is None:
                continue
            lo, hi = win
            sp = 1 - x.strand
            if any(y.a == x.a and y.strand == sp and lo - gp.band <= y.d <= hi + gp.band for y in accepted[1 - m]):
                continue
            tasks += 1
            o = revcomp_codes(codes[1 - m]) if sp else codes[1 - m]
            scores = window_scores(o, ref.codes[x.a], lo, hi, p.mismatch)
            d = lo + int(np.argmax(scores))  # (the first of the largest: the smallest d')
            if int(scores[d - lo]) >= p.min_score:
                score, b, e, nm = extend(o, ref.codes[x.a], d, p.mismatch)
                assert score == int(scores[d - lo]) and all((y.a, y.strand, y.d) != (x.a, sp, d) for y in accepted[1 - m])
                added[1 - m][(x.a, sp, d)] = Aln(x.a, sp, d, score, b, e, nm)
    return [list(added[0].values()), list(added[1].values())], tasks


def pair_list(accepted):
    """C_m: the accepted alignments of one mate by order_key under the overlap rule, the first PAIR_LIST of them."""
    kept = []
    for al in sorted(accepted, key=order_key):
        pos0, span = pos0_of(al), span_of(al)
        if any(x.a == al.a and x.strand == al.strand and pos0_of(x) < pos0 + span and pos0 < pos0_of(x) + span_of(x) for x in kept):
            continue
        kept.append(al)
        if len(kept) == PAIR_LIST:
            break
    return kept


def select_pair(acc1, L1, acc2, L2, p, pp):
    """The accepted alignments of the two mates (of L1 and L2 bases) -> (mate 1's kept ones, mate 2's, proper pair?)."""
    C, Ls, I = (pair_list(acc1), pair_list(acc2)), (L1, L2), pp.max_insert
    best = None
    for i, x in enumerate(C[0]):
        for j, y in enumerate(C[1]):
            if concordant(x, L1, y, L2, I) and (best is None or x.score + y.score > best[0]):
                best = (x.score + y.score, i, j)
    if best is None:
        return select(acc1, p), select(acc2, p), False
    out = []
    for m in (0, 1):
        kept = [C[m][best[1 + m]]]
        for t, x in enumerate(C[m]):
            if t == best[1 + m] or len(kept) == 1 + p.max_secondary:
                continue
            partners = [y.score for y in C[1 - m] if concordant(x, Ls[m], y, Ls[1 - m], I)]
            if partners and 100 * (x.score + max(partners)) >= p.sec_pct * best[0]:
                kept.append(x)
        out.append(kept)
    return out[0], out[1], True


def accepted_of(codes, index, ref, p):
    """One read's codes -> (its distinct candidates, its accepted alignments: ungapped Aln, in no order)."""
    cands = candidates(codes, index, p)
    rc, out = revcomp_codes(codes), []
    for a, strand, d in cands:
        score, b, e, nm = extend(rc if strand else codes, ref.codes[a], d, p.mismatch)
        if score >= p.min_score:
            out.append(Aln(a, strand, d, score, b, e, nm))
    return len(cands), out


def align_pair(seq1, seq2, index, ref, p, gp, pp):
    """The two mates' bytes -> (mate 1's kept alignments, mate 2's, proper pair?, distinct candidates, accepted candidates the
    rescued among them, refined candidates, rescued candidates, rescue tasks)."""
    codes = [refseq.codes_of(seq1), refseq.codes_of(seq2)]
    ncand, accepted = 0, []
    for c in codes:
        n, acc = accepted_of(c, index, ref, p)
        ncand += n
        accepted.append(acc)
    added, tasks = rescue_pair(codes, accepted, ref, p, gp, pp) if pp.rescue else ([[], []], 0)
    refined = 0
    for m in (0, 1):
        accepted[m] = accepted[m] + added[m]
        if gp.band > 0:
            for t, al in enumerate(accepted[m]):
                if al.e - al.b < len(codes[m]):
                    o = revcomp_codes(codes[m]) if al.strand else codes[m]
                    g = extend_gapped(o, ref.codes[al.a], al.d, p.mismatch, gp)
                    assert g[0] >= al.score, (g, al)
                    accepted[m][t] = GapAln(al.a, al.strand, al.d, *g)
                    refined += 1
    k1, k2, proper = select_pair(accepted[0], len(seq1), accepted[1], len(seq2), p, pp)
    return k1, k2, proper, ncand, len(accepted[0]) + len(accepted[1]), refined, len(added[0]) + len(added[1]), tasks


def align_reads_paired(seqs, ref, p, gp, pp, index=None):
    """Interleaved mates (an even number of reads) -> ([kept alignments per read], [proper? per pair], Stats, PairStats)."""
    if len(seqs) % 2:
        raise ValueError('an odd number of reads cannot be interleaved pairs')
    if index is None:
        index = build_index(ref, p.k, p.w)
    out, proper, ncand, nacc, nref, nres = [], [], 0, 0, 0, 0
    for i in range(0, len(seqs), 2):
        k1, k2, pr, c, a, r, x, _ = align_pair(seqs[i], seqs[i + 1], index, ref, p, gp, pp)
        out += [k1, k2]
        proper.append(pr)
        ncand += c
        nacc += a
        nref += r
        nres += x
    stats = Stats(len(seqs), sum(1 for x in out if x), ncand, nacc, sum(len(x) for x in out))
    return out, proper, stats, PairStats(nref, nres, sum(proper))


def pair_flag(mate, t, al, partner, proper):
    """The FLAG of record t (0: the primary) of mate `mate` (0 / 1); partner: the other mate's kept alignments."""
    return (1 + (2 if proper else 0) + (0 if partner else 8) + 16 * al.strand + (32 if partner and partner[0].strand else 0)
            + (128 if mate else 64) + (256 if t else 0))


def records(seqs, alns, proper=None):
    """What the device's batch holds for these reads and their kept alignments: (recs REC_DTYPE[], places, edits, bases entries,
    the pool's bytes).  proper: None, or for interleaved pairs one flag per pair (align_reads_paired)."""
    from ._hip import BASES_DTYPE, EDIT_DTYPE, PLACE_DTYPE, REC_DTYPE
    n = sum(len(x) for x in alns)
    recs, places = np.zeros(n, dtype=REC_DTYPE), np.zeros(n, dtype=PLACE_DTYPE)
    edits, entries = np.zeros(n, dtype=EDIT_DTYPE), np.zeros(n, dtype=BASES_DTYPE)
    pool = bytearray()
    r = 0
    for q, (seq, kept) in enumerate(zip(seqs, alns)):
        L = len(seq)
        for t, al in enumerate(kept):
            span, pos0, ops = span_of(al), pos0_of(al), ops_of(al)
            flag = 16 * al.strand + (256 if t else 0) if proper is None else pair_flag(q % 2, t, al, alns[q ^ 1], proper[q // 2])
            new = t == 0 and (proper is None or q % 2 == 0 or not alns[q - 1])  # (pairs: the first record of the pair)
            recs[r] = ((al.a | 0x80000000) if new else al.a, ops.count('M'), L + ops.count('D'), flag | ((0 if t else L) << 12))
            places[r] = (pos0, span)
            edits[r] = (al.nm, len(ops))
            if t == 0:
                codes = refseq.codes_of(seq)
                oriented = revcomp_codes(codes) if al.strand else codes
                o, i = [], al.b  # M: the read's code, D: GAP, I: skipped
                for op in ops:
                    if op != 'I':
                        o.append(GAP_CODE if op == 'D' else oriented[i])
                    i += op != 'D'
                assert len(o) == span and i == al.e
                entries[r] = (len(pool), pos0, span)
                pool += bytes(o[j] | ((o[j + 1] if j + 1 < span else 0) << 4) for j in range(0, span, 2))
            r += 1
    return recs, places, edits, entries, bytes(pool)


_COMP = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')
_LETTER = bytes(b if b in b'ACGTacgt' else ord('N') for b in range(256))


def sam_lines(headers, seqs, quals, names, lengths, alns, proper=None):
    """The alignments as SAM text (bytes lines with their newline).  headers: the reads' header lines without their first byte
    (QNAME: up to the first white byte); quals: the reads' qualities, or None for `*`; names, lengths: per accession row.
    proper: None, or for interleaved pairs one flag per pair: both mates get mate 1's QNAME without a trailing /1 or /2 and
    the pair's FLAG bits; RNEXT, PNEXT and TLEN stay `*`, 0, 0 and MAPQ 255."""
    out = [b'@SQ\tSN:%s\tLN:%d\n' % (nm.encode() if isinstance(nm, str) else nm, int(ln)) for nm, ln in zip(names, lengths)]
    for r, (hdr, seq, qual, kept) in enumerate(zip(headers, seqs, quals if quals is not None else [None] * len(seqs), alns)):
        if proper is not None:
            hdr = headers[r - r % 2]
        qname = bytes(hdr).split(None, 1)[0] if bytes(hdr).split(None, 1) else b'*'
        if proper is not None and qname[-2:] in (b'/1', b'/2') and len(qname) > 2:
            qname = qname[:-2]
        L = len(seq)
        for t, al in enumerate(kept):
            runs = [(m.group(0)[0], len(m.group(0))) for m in re.finditer(r'M+|I+|D+', ops_of(al))]
            cigar = (b'%dS' % al.b if al.b else b'') + b''.join(b'%d%s' % (n, op.encode()) for op, n in runs) + (b'%dS' % (L - al.e) if L - al.e else b'')
            if t == 0:
                s = bytes(seq).translate(_LETTER)
                q = bytes(qual) if qual is not None else b'*'
                if al.strand:
                    s = s.translate(_COMP)[::-1]
                    q = q[::-1] if qual is not None else q
            else:
                s = q = b'*'
            rname = names[al.a].encode() if isinstance(names[al.a], str) else names[al.a]
            flag = 16 * al.strand + (256 if t else 0) if proper is None else pair_flag(r % 2, t, al, alns[r ^ 1], proper[r // 2])
            out.append(b'\t'.join([qname, b'%d' % flag, rname, b'%d' % (pos0_of(al) + 1), b'255', cigar,
                                   b'*', b'0', b'0', s, q, b'NM:i:%d' % al.nm]) + b'\n')
    return out
