"""Per-genome breadth and depth of coverage from stage C's alignments (--coverage): the definition, on the host.

For every accession: how many alignments were placed on it, how many reference bases they span, and how many distinct
reference bases at least one of them covers.  Breadth (covered / length) set against the breadth the depth predicts
(1 - exp(-depth)) tells a genome that is there from a few hundred reads piled on one conserved region.

coverage(lines, acc2info, pct_id) reads SAM lines (str or bytes), header lines among them:

  Lengths.  Accession a has the LN of the LAST `@SQ` line whose SN is a.  An `@SQ` line counts only among the leading '@' lines
      and only with both an SN: and an LN: tag (LN a run of decimal digits).  Without one, a has acc2info[a][0] (db_info gives
      every accession of a taxid the FIRST accession's length, select_db.make_db_and_dbinfo: right only for one-contig genomes;
      the aligner's own header is right).  @SQ names db_info does not know are ignored.
  Which lines count.  A line the tokeniser retains (not '@', at least 6 fields of line.strip().split(), FLAG without 4, CIGAR not
      '*' — and it raises what the tokeniser raises), that clean_read_hits keeps (scripts/map_and_profile.py:130-147): FLAG without
      2048 and float(matched) / float(total) >= pct_id, matched and total being the record's own.  Secondary alignments count.
      What the read loop does with a line (the first line dropped after an Ambiguous read) plays no part.
  Placement.  pos0 = int(POS) - 1, POS being 1 to 10 ASCII digits with 1 <= POS <= 2^31 - 1 (anything else: not placed, never an
      error — the reference does not read POS).  span = the sum of the CIGAR's M, D, N and X lengths (at most 2^32 - 1: a larger sum
      stays there).  The alignment covers [pos0, min(pos0 + span, L)) AS ONE BLOCK: the bases under a D or N gap count as covered.
      A counting line with an unacceptable POS, span 0 or pos0 >= L is UNPLACED: one more in the unplaced count, nothing else.
  Per accession.  alignments = placed lines; aligned_bases = the sum of their clipped lengths; covered_bases = the size of the
      union of their intervals — by sorting and merging them here, by a bitmap on the device (mg_coverage.hip).

Everything is integer and independent of order, so the device is held to this exactly.
"""
import math
from collections import namedtuple

HEADER = '#kind\tid\ttaxid\tlength\talignments\taligned_bases\tcovered_bases\tbreadth\tmean_depth\texpected_breadth\n'
FLAG_MASK, MAX_SEQLEN, MAX_POS, MAX_SPAN = 0xFFF, (1 << 20) - 1, (1 << 31) - 1, (1 << 32) - 1

# lengths {accession: L}, per {accession: [alignments, aligned_bases, covered_bases]} (accessions with a placed line), unplaced
Coverage = namedtuple('Coverage', 'lengths per unplaced')


def _text(line):
    return bytes(line).decode('utf-8') if isinstance(line, (bytes, bytearray, memoryview)) else line


def sq_length(line):
    """An `@SQ` header line -> (SN, LN), None for any other line or one without both tags."""
    f = _text(line).rstrip('\r\n').split('\t')
    if f[0] != '@SQ':
        return None
    sn = ln = None
    for tag in f[1:]:
        if tag.startswith('SN:') and sn is None:
            sn = tag[3:]
        elif tag.startswith('LN:') and ln is None:
            ln = tag[3:]
    if not sn or not ln or not (ln.isascii() and ln.isdigit()):
        return None
    return sn, int(ln)


def lengths_of(header_lines, acc2info):
    """{accession: length}: db_info's, overridden by the `@SQ` lines (the last one of a name wins)."""
    lengths = {acc: int(info[0]) for acc, info in acc2info.items()}
    for line in header_lines:
        sq = sq_length(line)
        if sq is not None and sq[0] in lengths:
            lengths[sq[0]] = sq[1]
    return lengths


def span_of(cigar):
    """The reference bases a CIGAR consumes: M + D + N + X (a lower-case letter is an op of no kind, as for the tokeniser)."""
    span = num = 0
    for ch in cigar:
        if ch.isalpha():
            if ch in 'MDNX':
                span += num
            num = 0
        else:
            num = num * 10 + int(ch)
    return min(span, MAX_SPAN)


def placement(fields):
    """(pos0, span) of a retained line's fields; span = 0: not placed (then pos0 = 0)."""
    pos = fields[3]
    if not (1 <= len(pos) <= 10 and pos.isascii() and pos.isdigit()):
        return 0, 0
    pos = int(pos)
    if not 1 <= pos <= MAX_POS:
        return 0, 0
    span = span_of(fields[5])
    return (pos - 1, span) if span else (0, 0)


def retained_fields(line):
    """The fields of a line the tokeniser retains (map_and_profile._Tokeniser.feed), None for every other line."""
    line = _text(line)
    if line.startswith('@'):
        return None
    f = line.strip().split()
    if len(f) < 6:
        return None
    if (int(f[1]) & 4) or f[5] == '*':
        return None
    return f


def matched_total(f):
    """(matched, total) of the record of a retained line, with everything the tokeniser raises."""
    matched = total = num = 0
    for ch in f[5]:
        if ch.isalpha():
            if ch == 'M':
                matched += num
            total += num
            num = 0
        else:
            num = num * 10 + int(ch)  # '=' raises ValueError here, as in the reference
    int(f[11][5:])
    if total == 0:
        raise ZeroDivisionError('float division by zero')
    seqlen = 0 if f[9] == '*' else len(f[9])
    if seqlen > MAX_SEQLEN or matched > 0xFFFFFFFF or total > 0xFFFFFFFF:
        raise OverflowError('alignment longer than the record format allows')
    return matched, total


def counts(flag, matched, total, pct_id):
    """clean_read_hits keeps the line (:135)."""
    return not (flag & 2048) and float(matched) / float(total) >= pct_id


def union_size(intervals):
    """The number of integers in the union of half-open intervals [(begin, end)]: sorted and merged."""
    covered, cur_b, cur_e = 0, None, None
    for b, e in sorted(intervals):
        if cur_e is None or b > cur_e:
            if cur_e is not None:
                covered += cur_e - cur_b
            cur_b, cur_e = b, e
        elif e > cur_e:
            cur_e = e
    if cur_e is not None:
        covered += cur_e - cur_b
    return covered


def accumulate(placed, lengths):
    """[(accession, pos0, span)] of COUNTING lines -> (per {accession: [alignments, aligned_bases, covered_bases]}, unplaced)."""
    intervals, unplaced = {}, 0
    for acc, pos0, span in placed:
        L = lengths[acc]
        if span == 0 or pos0 >= L:
            unplaced += 1
            continue
        intervals.setdefault(acc, []).append((pos0, min(pos0 + span, L)))
    per = {}
    for acc, iv in intervals.items():
        per[acc] = [len(iv), sum(e - b for b, e in iv), union_size(iv)]
    return per, unplaced


def coverage(lines, acc2info, pct_id):
    """SAM lines (str or bytes; the header among them) -> Coverage(lengths, per, unplaced)."""
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
        acc2info[f[2]]  # KeyError for an RNAME db_info does not know (:217)
        matched, total = matched_total(f)
        if not counts(int(f[1]), matched, total, pct_id):
            continue
        placed.append((f[2],) + placement(f))
    lengths = lengths_of(header, acc2info)
    per, unplaced = accumulate(placed, lengths)
    return Coverage(lengths, per, unplaced)


def coverage_of_records(recs, places, accessions, lengths, pct_id):
    """The same from (record, place) pairs: recs with the fields of mg_aln_rec (ref_new, matched, total, flag_len), places
    (pos0, span) per record, accessions[row] the name of accession row `ref_new & 0x7fffffff` -> Coverage.  A counting record whose row is at or beyond the
    accessions is unplaced, as on the device."""
    placed, no_row = [], 0
    for r, (pos0, span) in zip(recs, places):
        flag = int(r['flag_len']) & FLAG_MASK
        if not counts(flag, int(r['matched']), int(r['total']), pct_id):
            continue
        row = int(r['ref_new']) & 0x7FFFFFFF
        if row >= len(accessions):  # (no such accession: the device counts the record as unplaced)
            no_row += 1
            continue
        placed.append((accessions[row], int(pos0), int(span)))
    per, unplaced = accumulate(placed, lengths)
    return Coverage(lengths, per, unplaced + no_row)


def rows(cov, acc2info, taxid2info):
    """-> [(kind, id, taxid, length, alignments, aligned_bases, covered_bases)]: an 'S' row per accession with a placed alignment
    in db_info order, then a 'G' row per taxid that has one, in taxid2info order — its length the sum over ALL its accessions."""
    out, by_tax = [], {}
    for acc, info in acc2info.items():
        g = by_tax.setdefault(info[1], [0, 0, 0, 0])
        g[0] += cov.lengths[acc]
        st = cov.per.get(acc)
        if st is None:
            continue
        out.append(('S', acc, info[1], cov.lengths[acc]) + tuple(st))
        for i in range(3):
            g[1 + i] += st[i]
    for taxid in taxid2info:
        g = by_tax.get(taxid)
        if g is not None and g[1] >= 1:
            out.append(('G', taxid, taxid) + tuple(g))
    return out


def format_row(row):
    kind, ident, taxid, length, alignments, aligned, covered = row
    breadth = covered / length if length else 0.0
    depth = aligned / length if length else 0.0
    return '%s\t%s\t%s\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\n' % (kind, ident, taxid, length, alignments, aligned, covered, breadth,
                                                            depth, 1.0 - math.exp(-depth))


def format_block(block_rows, unplaced, source=None):
    """One input file's block: `#file\\t<source>` (several input files only), its rows, `#unplaced\\t<n>`."""
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_row(r) for r in block_rows) + '#unplaced\t%d\n' % unplaced


def write_coverage(path, block_rows=None, unplaced=0, source=None, append=False):
    """TSV: the column header (a new file only), then — unless block_rows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER)
        if block_rows is not None:
            out.write(format_block(block_rows, unplaced, source))
