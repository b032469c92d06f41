"""Short reads aligned to the reference FASTA by seed and extend (--aligner device): the definition, on the host.

This is NOT a port of minimap2 and claims no parity with it: it is a small aligner of its own, defined here so that the device
(mg_align.hip; the per-position rules are in mg_align_core.h and mg_align_gap_core.h) can be held to it exactly.  Without
--align_band it is UNGAPPED: a read whose only good alignment needs an insertion or deletion aligns in part or not at all.  With
--align_band B > 0 a candidate whose ungapped segment is shorter than its read is refined by a banded local alignment with affine
gaps (extend_gapped), which finds insertions and deletions of up to B bases.  It knows no pairs, keeps no names and gives no MAPQ.
Every read counts as its own read: each primary record carries the new-read bit, whatever the read's name — two reads of one
name (the mates of a pair in one file) are two reads.

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


def records(seqs, alns):
    """What the device's batch holds for these reads and their kept alignments: (recs REC_DTYPE[], places, edits, bases entries,
    the pool's bytes)."""
    from ._hip import BASES_DTYPE, EDIT_DTYPE, PLACE_DTYPE, REC_DTYPE
    n = sum(len(x) for x in alns)
    recs, places = np.zeros(n, dtype=REC_DTYPE), np.zeros(n, dtype=PLACE_DTYPE)
    edits, entries = np.zeros(n, dtype=EDIT_DTYPE), np.zeros(n, dtype=BASES_DTYPE)
    pool = bytearray()
    r = 0
    for seq, kept in zip(seqs, alns):
        L = len(seq)
        for t, al in enumerate(kept):
            span, pos0, ops = span_of(al), pos0_of(al), ops_of(al)
            recs[r] = ((al.a | 0x80000000) if t == 0 else al.a, ops.count('M'), L + ops.count('D'), (16 * al.strand + (256 if t else 0)) | ((0 if t else L) << 12))
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


def sam_lines(headers, seqs, quals, names, lengths, alns):
    """The alignments as SAM text (bytes lines with their newline).  headers: the reads' header lines without their first byte
    (QNAME: up to the first white byte); quals: the reads' qualities, or None for `*`; names, lengths: per accession row."""
    out = [b'@SQ\tSN:%s\tLN:%d\n' % (nm.encode() if isinstance(nm, str) else nm, int(ln)) for nm, ln in zip(names, lengths)]
    for hdr, seq, qual, kept in zip(headers, seqs, quals if quals is not None else [None] * len(seqs), alns):
        qname = bytes(hdr).split(None, 1)[0] if bytes(hdr).split(None, 1) else b'*'
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
            out.append(b'\t'.join([qname, b'%d' % (16 * al.strand + (256 if t else 0)), rname, b'%d' % (pos0_of(al) + 1), b'255', cigar,
                                   b'*', b'0', b'0', s, q, b'NM:i:%d' % al.nm]) + b'\n')
    return out
