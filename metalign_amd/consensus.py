"""The consensus sequence per accession from stage C's pileup (--consensus): the definition, on the host.

--variants piles the read bases on the reference and prints aggregates of the counts; this writes the sequence the sample carries for
every detected accession, as FASTA.  Which lines count, how a line is piled and the counts n[acc][pos][code] are variants.py's (its
functions are used, not restated), and so are the thresholds (D, C, F) = variants.params and the site rule variants.site_of.  On top:

  Site character (char_of).  d = nA + nC + nG + nT.  d < D: `N`.  Else, mode `major`: LETTERS[major], ties to the lowest code as
      site_of breaks them; mode `iupac`: IUPAC[mask], mask = 1 << major or'ed with the bits of site_of's variant alleles (A = 1,
      C = 2, G = 4, T = 8).  A callable site that is not polymorphic gives the same letter in both modes; a site that reads only skip
      or cover with other bytes has d = 0 and is `N`.  The sequence keeps the reference's coordinates: its length is always L.
  Text (text_of).  The bases with a `\\n` behind every `width` of them and behind the last one: L + ceil(L / width) bytes, no empty
      last line, nothing for L = 0.  The files use LINE_WIDTH.
  Which accessions.  Those with a piled alignment, in db_info order (the S rows of --variants), and of them those with
      1000 * callable_sites >= M * L, M = int(round(min_called * 1000)) (min_called_permille).  Integers only.
  Record.  `>ACC taxid=T length=L alignments=n called=callable_sites ambiguous=polymorphic_sites min_depth=D min_count=C
      min_freq_permille=F ambiguity=major|iupac`, then ` reads=unique` under --side_reads unique, then ` file=SOURCE` where there
      are several input files; then the text.  called and ambiguous are what --variants prints for the accession.

FASTA has no comment lines: a new file is empty, and nothing else is ever written at its top.  Everything is integer and independent
of order, so the device (mg_variants.hip: k_var_consensus) is held to this byte for byte.
"""
from collections import namedtuple

from . import variants

IUPAC = '-ACMGRSVTWYHKDBN'
MODES = ('major', 'iupac')
LINE_WIDTH = 60
SLAB_BYTES = 64 << 20  # the text the driver fetches from the device in one call, at the most (a row longer than this is a slab)

# seq: bytes, L of them
Record = namedtuple('Record', 'acc taxid length alignments called ambiguous seq')


def min_called_permille(min_called=0.0):
    """M of --consensus_min_called; ValueError out of range."""
    f = float(min_called)
    if not 0.0 <= f <= 1.0:
        raise ValueError('--consensus_min_called must lie within 0 to 1.')
    return int(round(f * 1000))


def char_of(n4, p, iupac):
    """One site's four counts -> its character."""
    ok, major, var, _, _ = variants.site_of(n4, p)
    if not ok:
        return 'N'
    return IUPAC[(1 << major) | sum(1 << a for a in var)] if iupac else variants.LETTERS[major]


def text_bytes(L, width=LINE_WIDTH):
    return L + (L + width - 1) // width


def text_of(seq, width=LINE_WIDTH):
    """bytes of bases -> bytes of text."""
    return b''.join(seq[i:i + width] + b'\n' for i in range(0, len(seq), width))


def written(length, called, permille):
    """The --consensus_min_called test of an accession that has a piled alignment."""
    return 1000 * called >= permille * length


def records_of(n, aln, unpiled, lengths, order, acc2info, p, iupac, min_called=0.0):
    """accumulate()'s three -> [Record], in `order`."""
    M = min_called_permille(min_called)
    per = variants.summarise(n, aln, unpiled, lengths, order, p).per
    out = []
    for acc in order:
        st = per.get(acc)
        if st is None or st[0] < 1 or not written(lengths[acc], st[1], M):
            continue
        seq = bytearray(b'N' * lengths[acc])
        for pos, n4 in n.get(acc, {}).items():
            seq[pos] = ord(char_of(n4, p, iupac))
        out.append(Record(acc, acc2info[acc][1], lengths[acc], st[0], st[1], st[2], bytes(seq)))
    return out


def consensus(lines, acc2info, pct_id, p=None, iupac=False, min_called=0.0):
    """SAM lines (str or bytes; the header among them) -> [Record]."""
    n, aln, unpiled, lengths = variants.counts_of_lines(lines, acc2info, pct_id)
    return records_of(n, aln, unpiled, lengths, list(acc2info), acc2info, p or variants.params(), iupac, min_called)


def consensus_of_records(recs, entries, pool, accessions, lengths, pct_id, acc2info, p=None, iupac=False, min_called=0.0):
    """The same as consensus() from records; the order of db_info is the order of `accessions`."""
    n, aln, unpiled = variants.counts_of_records(recs, entries, pool, accessions, lengths, pct_id)
    return records_of(n, aln, unpiled, lengths, list(accessions), acc2info, p or variants.params(), iupac, min_called)


def header_line(acc, taxid, length, alignments, called, ambiguous, p, iupac, unique=False, source=None):
    return '>%s taxid=%s length=%d alignments=%d called=%d ambiguous=%d min_depth=%d min_count=%d min_freq_permille=%d ambiguity=%s%s%s\n' % (
        acc, taxid, length, alignments, called, ambiguous, p.min_depth, p.min_count, p.permille, MODES[bool(iupac)],
        ' reads=unique' if unique else '', ' file=%s' % source if source is not None else '')


def format_record(rec, p, iupac, unique=False, source=None, width=LINE_WIDTH):
    """-> bytes: the header line and the text."""
    return header_line(*rec[:6], p, iupac, unique, source).encode('utf-8') + text_of(rec.seq, width)


def write_consensus(path, records=None, append=False, p=None, iupac=False, unique=False, source=None):
    """FASTA: a new file is created empty; then — unless records is None — one input file's records."""
    with open(path, 'ab' if append else 'wb') as out:
        for rec in records or ():
            out.write(format_record(rec, p or variants.params(), iupac, unique, source))


def slabs(text_sizes, slab_bytes=None):
    """[(first, end)]: consecutive texts of these sizes grouped into slabs of up to slab_bytes (SLAB_BYTES); a slab holds at least
    one text however long."""
    limit = SLAB_BYTES if slab_bytes is None else slab_bytes
    out, first, held = [], 0, 0
    for i, size in enumerate(text_sizes):
        if i > first and held + size > limit:
            out.append((first, i))
            first, held = i, 0
        held += size
    if len(text_sizes) > first:
        out.append((first, len(text_sizes)))
    return out
