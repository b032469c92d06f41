"""Alignment identity per genome from stage C's alignments (--identity): the definition, on the host.

Breadth and depth say how many reads a genome took and where they lie; identity says how well they match it — the database's
strain, or a 94 % relative that happened to be the nearest genome.  Which lines count is coverage.py's rule (its functions are used,
not restated).  On top of it:

  Edit of a retained line (edit_of).  cols = the sum of the CIGAR's M, I, D and X lengths, at most 2^32 - 1 (a lower-case letter is
      an op of no kind, as in coverage.span_of; '=' never gets here: matched_total raises on it).  nm comes from the FIRST field t of
      f[11:] (the fields of line.strip().split()) with t.startswith('NM:i:'), and the search stops there: with v = t[5:], nm = int(v)
      when v is an optional sign and at least one ASCII digit and 0 <= int(v) <= 2^32 - 2 (leading zeros are fine); anything else —
      no such field, an empty, malformed or negative value, one too large — is NONE = 2^32 - 1.
  Scored.  A counting line with nm != NONE and cols > 0 (from records: and an accession row < nacc).  Every other counting line is
      one more in `unscored` and nothing else.
  Per scored line.  e = min(nm, cols); bin = (cols - e) * 1000 // cols, 0 .. 1000.
  Per accession.  alignments, columns = sum(cols), edits = sum(e), H[bin].  A genome sums its accessions.
  Statistics (stats), from columns, edits and H alone, exact: identity = 1 - edits / columns; median_identity = the bin that holds
      ascending rank (n - 1) // 2, p10_identity the one that holds rank n // 10, both printed as bin / 1000; aln_ge_900 / 950 / 970 /
      990 = the alignments with bin >= that value.

Everything is integer and independent of order, so the device (mg_identity.hip) is held to this exactly.
"""
from collections import namedtuple
from fractions import Fraction

from .coverage import FLAG_MASK, _text, counts, matched_total, retained_fields

NONE, MAX_NM, MAX_COLS, BINS = (1 << 32) - 1, (1 << 32) - 2, (1 << 32) - 1, 1001
HEADER = ('#kind\tid\ttaxid\talignments\taligned_columns\tedit_distance\tidentity\tmedian_identity\tp10_identity\taln_ge_900'
          '\taln_ge_950\taln_ge_970\taln_ge_990\n')

# per {accession: [alignments, columns, edits, {bin: alignments}]} (accessions with a scored line); unscored
Identity = namedtuple('Identity', 'per unscored')
Stats = namedtuple('Stats', 'identity median p10 ge900 ge950 ge970 ge990')


def cols_of(cigar):
    """The alignment columns of a CIGAR: M + I + D + X."""
    cols = num = 0
    for ch in cigar:
        if ch.isalpha():
            if ch in 'MIDX':
                cols += num
            num = 0
        else:
            num = num * 10 + int(ch)
    return min(cols, MAX_COLS)


def nm_of(tags):
    """The fields from the twelfth on -> the value of the first `NM:i:` field, NONE when there is no usable one."""
    for t in tags:
        if not t.startswith('NM:i:'):
            continue
        v = t[5:]
        digits = v[1:] if v[:1] in ('+', '-') else v
        if not digits or not all('0' <= ch <= '9' for ch in digits):
            return NONE
        n = int(v)
        return n if 0 <= n <= MAX_NM else NONE
    return NONE


def edit_of(fields):
    """(nm, cols) of a retained line's fields."""
    return nm_of(fields[11:]), cols_of(fields[5])


def accumulate(edits):
    """[(accession, nm, cols)] of COUNTING lines -> Identity."""
    per, unscored = {}, 0
    for acc, nm, cols in edits:
        if nm == NONE or cols == 0:
            unscored += 1
            continue
        e = min(nm, cols)
        st = per.setdefault(acc, [0, 0, 0, {}])
        st[0] += 1
        st[1] += cols
        st[2] += e
        b = (cols - e) * 1000 // cols
        st[3][b] = st[3].get(b, 0) + 1
    return Identity(per, unscored)


def identity(lines, acc2info, pct_id):
    """SAM lines (str or bytes; header lines among them) -> Identity."""
    edits = []
    for line in lines:
        f = retained_fields(line)
        if f is None:
            continue
        acc2info[f[2]]  # KeyError for an RNAME db_info does not know, as coverage
        matched, total = matched_total(f)
        if not counts(int(f[1]), matched, total, pct_id):
            continue
        edits.append((f[2],) + edit_of(f))
    return accumulate(edits)


def identity_of_records(recs, edits, accessions, pct_id):
    """The same from (record, edit) pairs: recs with the fields of mg_aln_rec, edits (nm, cols) per record, accessions[row] the name
    of accession row `ref_new & 0x7fffffff` (a row beyond them: unscored, as on the device)."""
    got, no_row = [], 0
    for r, (nm, cols) in zip(recs, edits):
        if not counts(int(r['flag_len']) & FLAG_MASK, int(r['matched']), int(r['total']), pct_id):
            continue
        row = int(r['ref_new']) & 0x7FFFFFFF
        if row >= len(accessions):
            no_row += 1
            continue
        got.append((accessions[row], int(nm), int(cols)))
    idn = accumulate(got)
    return Identity(idn.per, idn.unscored + no_row)


def _bin_at(bins, rank):
    at = 0
    for b, n in bins:
        if at + n > rank:
            return b
        at += n
    return bins[-1][0]


def stats(columns, edits, H):
    """-> Stats, exact; without alignments zeros."""
    bins = sorted((b, n) for b, n in H.items() if n)
    n = sum(c for _, c in bins)
    if n == 0 or columns == 0:
        return Stats(Fraction(0), 0, 0, 0, 0, 0, 0)
    ge = [sum(c for b, c in bins if b >= k) for k in (900, 950, 970, 990)]
    return Stats(1 - Fraction(edits, columns), _bin_at(bins, (n - 1) // 2), _bin_at(bins, n // 10), *ge)


def rows(idn, acc2info, taxid2info):
    """-> [(kind, id, taxid, alignments, columns, edits, H)]: an 'S' row per accession with a scored alignment in db_info order, then
    a 'G' row per taxid that has one, in taxid2info order (the order of coverage.rows)."""
    out, by_tax = [], {}
    for acc, info in acc2info.items():
        st = idn.per.get(acc)
        if st is None or st[0] < 1:
            continue
        out.append(('S', acc, info[1], st[0], st[1], st[2], st[3]))
        g = by_tax.setdefault(info[1], [0, 0, 0, {}])
        for i in range(3):
            g[i] += st[i]
        for b, n in st[3].items():
            g[3][b] = g[3].get(b, 0) + n
    for taxid in taxid2info:
        g = by_tax.get(taxid)
        if g is not None and g[0] >= 1:
            out.append(('G', taxid, taxid) + tuple(g))
    return out


def format_row(row):
    kind, ident, taxid, alignments, columns, edits, H = row
    s = stats(columns, edits, H)
    return '%s\t%s\t%s\t%d\t%d\t%d\t%.6f\t%.3f\t%.3f\t%d\t%d\t%d\t%d\n' % (
        kind, ident, taxid, alignments, columns, edits, float(s.identity), s.median / 1000, s.p10 / 1000, s.ge900, s.ge950, s.ge970,
        s.ge990)


def format_block(block_rows, unscored, source=None):
    """One input file's block: `#file\\t<source>` (several input files only), its rows, `#unscored\\t<n>`."""
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_row(r) for r in block_rows) + '#unscored\t%d\n' % unscored


def write_identity(path, block_rows=None, unscored=0, source=None, append=False):
    """TSV: the column header (a new file only), then — unless block_rows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER)
        if block_rows is not None:
            out.write(format_block(block_rows, unscored, source))
