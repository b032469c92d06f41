"""Per-site allele counts and strain diversity from stage C's alignments (--variants, --variant_sites): the definition, on the host.

Coverage, depth and identity say how much of a genome the reads cover, how deep and how closely; none looks at the read bases.
This one piles them on the reference: per reference base the reads' A, C, G and T, and from those whether a genome in the sample
is one strain or a mixture (nucleotide diversity pi, polymorphic sites per kb) and where the sample differs.  Which lines count
is coverage.py's rule (its functions are used, not restated).  On top of it:

  Pile of a counting line (pile_of).  (pos0, span) = coverage.placement.  The CIGAR is walked number and letter: M and X consume a
      query base and a reference base and emit the base's code; I and S consume query bases only; D and N consume reference bases
      and emit GAP = 5; H, P and every other letter (a lower-case one included) consume nothing.  Codes: A a = 0, C c = 1, G g = 2,
      T t = 3, every other byte OTHER = 4.  SEQ is taken as bytes.
  Piled.  span > 0, SEQ is not `*`, the query bases M, X, I and S consume equal len(SEQ), span <= MAX_PILE_SPAN = 2^21 - 1 — that
      much a line says by itself (bases_of) — and pos0 < L, L from coverage.lengths_of (from records: and an accession row < nacc).
      Every other counting line is one more in `unpiled` and nothing else.
  Counts.  A piled line adds 1 to n[acc][pos0 + j][code] for every j < span with pos0 + j < L and code < 4; alignments[acc] = its
      piled lines.
  Sites (site_of), with D = min_depth, C = min_count, F = int(round(min_freq * 1000)): d = nA + nC + nG + nT; d >= D: CALLABLE;
      the major allele has the largest count, ties to the lowest code; another allele a is a VARIANT allele when n_a >= C and
      1000 n_a >= F d; a callable site with a variant allele is POLYMORPHIC.
  Per accession.  callable_sites, polymorphic_sites, pairs = sum d (d - 1) and discordant = sum (d (d - 1) - sum_i n_i (n_i - 1))
      over the callable sites.  A genome sums its accessions.  pi = discordant / pairs, snv_per_kb = 1000 polymorphic / callable,
      both exact (Fractions) until they are printed.

Everything is integer and independent of order, so the device (mg_variants.hip) is held to this exactly.
"""
from collections import namedtuple
from fractions import Fraction

from .coverage import FLAG_MASK, _text, counts, lengths_of, matched_total, placement, retained_fields

OTHER, GAP, MAX_PILE_SPAN = 4, 5, (1 << 21) - 1
LETTERS = 'ACGT'
HEADER = ('#kind\tid\ttaxid\tlength\talignments\tcallable_sites\tpolymorphic_sites\tpairs\tdiscordant_pairs\tpi\tsnv_per_kb\n')
SITES_HEADER = '#accession\tpos\tdepth\tA\tC\tG\tT\tmajor\tvariant_alleles\n'
_CODE = {ord(c): i for i, c in enumerate(LETTERS)}
_CODE.update({ord(c.lower()): i for i, c in enumerate(LETTERS)})

# lengths {accession: L}; per {accession: [alignments, callable, polymorphic, pairs, discordant]} (accessions with a piled line);
# sites [(accession, pos0, (nA, nC, nG, nT))] — the polymorphic ones, in db_info order, then by position; unpiled
Variants = namedtuple('Variants', 'lengths per sites unpiled')
Params = namedtuple('Params', 'min_depth min_count permille')


def params(min_depth=5, min_count=2, min_freq=0.05):
    """(D, C, F) of the three flags; ValueError out of range."""
    D, C, f = int(min_depth), int(min_count), float(min_freq)
    if D < 2:
        raise ValueError('--variant_min_depth must be at least 2.')
    if C < 1:
        raise ValueError('--variant_min_count must be at least 1.')
    if not 0.0 <= f <= 0.5:
        raise ValueError('--variant_min_freq must lie within 0 to 0.5.')
    return Params(D, C, int(round(f * 1000)))


def params_line(p):
    return '#min_depth\t%d\tmin_count\t%d\tmin_freq_permille\t%d\n' % tuple(p)


def code_of(byte):
    return _CODE.get(byte, OTHER)


def _ops(cigar):
    """[(number, letter)] of a CIGAR, as coverage.span_of reads it."""
    ops, num = [], 0
    for ch in cigar:
        if ch.isalpha():
            ops.append((num, ch))
            num = 0
        else:
            num = num * 10 + int(ch)
    return ops


def bases_of(fields):
    """(pos0, span, codes) of a retained line's fields, what a line says by itself: span = 0 (then pos0 = 0, codes = []) when it
    cannot be piled; else codes[j] is what the line puts on reference base pos0 + j."""
    pos0, span = placement(fields)
    seq = fields[9].encode('utf-8')
    if span == 0 or span > MAX_PILE_SPAN or seq == b'*':
        return 0, 0, []
    ops = _ops(fields[5])
    if sum(n for n, op in ops if op in 'MXIS') != len(seq):
        return 0, 0, []
    codes, q = [], 0
    for n, op in ops:
        if op in 'MX':
            codes.extend(code_of(b) for b in seq[q:q + n])
            q += n
        elif op in 'IS':
            q += n
        elif op in 'DN':
            codes.extend([GAP] * n)
    assert len(codes) == span
    return pos0, span, codes


def pack(codes):
    """4-bit codes -> bytes, two per byte with the low nibble first; the unused high nibble of an odd count is 0."""
    out = bytearray((len(codes) + 1) // 2)
    for j, c in enumerate(codes):
        out[j >> 1] |= c << (4 * (j & 1))
    return bytes(out)


def unpack(data, span):
    return [(data[j >> 1] >> (4 * (j & 1))) & 15 for j in range(span)]


def entries_and_pool(all_fields):
    """The side array of a batch: [(off, pos0, span)] per retained line and the pool its codes lie in (mg_aln_bases)."""
    entries, pool = [], bytearray()
    for f in all_fields:
        pos0, span, codes = bases_of(f)
        entries.append((len(pool) if span else 0, pos0, span))
        pool += pack(codes)
    return entries, bytes(pool)


def accumulate(piles, lengths):
    """[(accession, pos0, span, codes)] of COUNTING lines -> (n {accession: {pos: [nA, nC, nG, nT]}}, alignments {accession: n},
    unpiled)."""
    n, aln, unpiled = {}, {}, 0
    for acc, pos0, span, codes in piles:
        L = lengths[acc]
        if span == 0 or pos0 >= L:
            unpiled += 1
            continue
        aln[acc] = aln.get(acc, 0) + 1
        at = n.setdefault(acc, {})
        for j in range(min(span, L - pos0)):
            if codes[j] < 4:
                at.setdefault(pos0 + j, [0, 0, 0, 0])[codes[j]] += 1
    return n, aln, unpiled


def site_of(n4, p):
    """One site's four counts -> (callable, major, [variant alleles], pairs, discordant); pairs and discordant are those of a
    callable site, 0 otherwise."""
    d = sum(n4)
    if d < p.min_depth:
        return False, 0, [], 0, 0
    major = max(range(4), key=lambda i: (n4[i], -i))
    var = [a for a in range(4) if a != major and n4[a] >= p.min_count and 1000 * n4[a] >= p.permille * d]
    pairs = d * (d - 1)
    return True, major, var, pairs, pairs - sum(x * (x - 1) for x in n4)


def summarise(n, aln, unpiled, lengths, order, p):
    """The counts -> Variants.  order: the accessions in db_info order."""
    per, sites = {}, []
    for acc in order:
        if not aln.get(acc):
            continue
        st = [aln[acc], 0, 0, 0, 0]
        for pos in sorted(n.get(acc, {})):
            n4 = n[acc][pos]
            ok, _, var, pairs, disc = site_of(n4, p)
            if not ok:
                continue
            st[1] += 1
            st[3] += pairs
            st[4] += disc
            if var:
                st[2] += 1
                sites.append((acc, pos, tuple(n4)))
        per[acc] = st
    return Variants(lengths, per, sites, unpiled)


def counts_of_lines(lines, acc2info, pct_id):
    """SAM lines (str or bytes; the header among them) -> accumulate()'s three and the lengths."""
    header, piles, leading = [], [], True
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
        piles.append((f[2],) + bases_of(f))
    lengths = lengths_of(header, acc2info)
    return accumulate(piles, lengths) + (lengths,)


def variants(lines, acc2info, pct_id, p=None):
    """SAM lines (str or bytes; the header among them) -> Variants."""
    n, aln, unpiled, lengths = counts_of_lines(lines, acc2info, pct_id)
    return summarise(n, aln, unpiled, lengths, list(acc2info), p or params())


def counts_of_records(recs, entries, pool, accessions, lengths, pct_id):
    """(record, entry) pairs and the pool -> accumulate()'s three: recs with the fields of mg_aln_rec, entries (off, pos0, span) per
    record, accessions[row] the name of accession row `ref_new & 0x7fffffff` (a row beyond them: unpiled, as on the device)."""
    piles, no_row = [], 0
    for r, (off, pos0, span) in zip(recs, entries):
        if not counts(int(r['flag_len']) & FLAG_MASK, int(r['matched']), int(r['total']), pct_id):
            continue
        row = int(r['ref_new']) & 0x7FFFFFFF
        if row >= len(accessions):
            no_row += 1
            continue
        off, pos0, span = int(off), int(pos0), int(span)
        piles.append((accessions[row], pos0, span, unpack(pool[off:off + (span + 1) // 2], span)))
    n, aln, unpiled = accumulate(piles, lengths)
    return n, aln, unpiled + no_row


def variants_of_records(recs, entries, pool, accessions, lengths, pct_id, p=None):
    """The same as variants() from records; the order of db_info is the order of `accessions`."""
    n, aln, unpiled = counts_of_records(recs, entries, pool, accessions, lengths, pct_id)
    return summarise(n, aln, unpiled, lengths, list(accessions), p or params())


def rows(var, acc2info, taxid2info):
    """-> [(kind, id, taxid, length, alignments, callable, polymorphic, pairs, discordant)]: an 'S' row per accession with a piled
    alignment in db_info order, then a 'G' row per taxid that has one, in taxid2info order — its length the sum over ALL its
    accessions (the order and the lengths of coverage.rows)."""
    out, by_tax = [], {}
    for acc, info in acc2info.items():
        g = by_tax.setdefault(info[1], [0, 0, 0, 0, 0, 0])
        g[0] += var.lengths[acc]
        st = var.per.get(acc)
        if st is None or st[0] < 1:
            continue
        out.append(('S', acc, info[1], var.lengths[acc]) + tuple(st))
        for i in range(5):
            g[1 + i] += st[i]
    for taxid in taxid2info:
        g = by_tax.get(taxid)
        if g is not None and g[1] >= 1:
            out.append(('G', taxid, taxid) + tuple(g))
    return out


def ratios(callable_sites, polymorphic, pairs, discordant):
    """-> (pi, snv_per_kb), exact; 0 where the denominator is."""
    return (Fraction(discordant, pairs) if pairs else Fraction(0),
            Fraction(1000 * polymorphic, callable_sites) if callable_sites else Fraction(0))


def format_row(row):
    kind, ident, taxid, length, aln, call, poly, pairs, disc = row
    pi, snv = ratios(call, poly, pairs, disc)
    return '%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\n' % (kind, ident, taxid, length, aln, call, poly, pairs, disc, float(pi),
                                                                   float(snv))


def format_block(block_rows, unpiled, source=None):
    """One input file's block: `#file\\t<source>` (several input files only), its rows, `#unpiled\\t<n>`."""
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_row(r) for r in block_rows) + '#unpiled\t%d\n' % unpiled


def write_variants(path, p=None, block_rows=None, unpiled=0, source=None, append=False):
    """TSV: the column header and the line that names D, C and F (a new file only), then — unless block_rows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER + params_line(p or params()))
        if block_rows is not None:
            out.write(format_block(block_rows, unpiled, source))


def format_site(site, p):
    acc, pos0, n4 = site
    _, major, var, _, _ = site_of(n4, p)
    return '%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n' % (acc, pos0 + 1, sum(n4), n4[0], n4[1], n4[2], n4[3], LETTERS[major],
                                                   ','.join(LETTERS[a] for a in var))


def write_sites(path, p=None, sites=None, source=None, append=False):
    """TSV: the column header and the parameters' line (a new file only), then — unless sites is None — one input file's rows,
    one per polymorphic site, behind `#file\\t<source>` where there are several input files."""
    p = p or params()
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(SITES_HEADER + params_line(p))
        if sites is not None:
            if source is not None:
                out.write('#file\t%s\n' % source)
            out.writelines(format_site(s, p) for s in sites)
