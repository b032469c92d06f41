"""The reference bases per accession from the bytes of a FASTA file (--ani, --vcf): the definition, on the host.

The pileup of variants.py never sees the reference base; this gives it, per accession row, as the codes of variants.code_of.  It is
defined on BYTES, never through Python's text mode, so no file is left undecided:

  Lines.  The file is split at `\\n`; a last line needs no `\\n`.
  Records.  A line whose first byte is `>` opens a record; its name is the bytes behind the `>` up to the first space, tab, `\\r`,
      `\\v` or `\\f` (what an aligner writes as RNAME).  Lines in front of the first header are dropped.  Every other line is stripped
      of space, tab, `\\r`, `\\v` and `\\f` at both ends and its bytes are appended to the open record: bytes inside the line are kept
      and coded.
  Codes.  variants.code_of: ACGTacgt are 0..3, every other byte OTHER = 4.
  Kinds.  With acc_index {name: row} and the lengths the accumulators are sized by (coverage.lengths_of), a record is LOADED when its
      name is a row and it has exactly that row's length in bases; `foreign` when its name is no row (an empty name is none);
      `mismatched` when it names a row of another length — the row then stays without a reference; `duplicate` when an earlier
      record already loaded or mismatched its row: the first record wins.  A row of length 0 is loaded by a record without bases.

Everything is bytes and integers, so the device (mg_refseq.hip) is held to this exactly.
"""
from collections import namedtuple

from .variants import OTHER, code_of

WHITE = b' \t\r\v\f'
_WHITE = frozenset(WHITE)
_TABLE = bytes(code_of(b) for b in range(256))

# counters: every record is exactly one of loaded, foreign, mismatched, duplicate
Counters = namedtuple('Counters', 'records loaded foreign mismatched duplicate')
# codes {row: bytes of codes} of the loaded rows; loaded[row] 0 / 1
RefSeq = namedtuple('RefSeq', 'codes loaded counters')


def name_of(line):
    """A header line (without its `\\n`) -> the record's name, bytes."""
    end = 1
    while end < len(line) and line[end] not in _WHITE:
        end += 1
    return line[1:end]


def records_of(data):
    """FASTA bytes -> [(name, bases)], both bytes."""
    out = []
    for line in bytes(data).split(b'\n'):
        if line[:1] == b'>':
            out.append((name_of(line), []))
        elif out:
            out[-1][1].append(line.strip(WHITE))
    return [(name, b''.join(parts)) for name, parts in out]


def codes_of(bases):
    return bytes(bases).translate(_TABLE)


def parse(data, acc_index, lengths):
    """FASTA bytes, {name (str or bytes): row}, lengths[row] -> RefSeq."""
    rows = {(a.encode('utf-8') if isinstance(a, str) else bytes(a)): int(i) for a, i in acc_index.items()}
    codes, seen = {}, set()
    loaded = [0] * len(lengths)
    n = [0, 0, 0, 0, 0]
    for name, bases in records_of(data):
        n[0] += 1
        row = rows.get(name) if name else None
        if row is None:
            n[2] += 1
        elif row in seen:
            n[4] += 1
        elif len(bases) == int(lengths[row]):
            seen.add(row)
            codes[row], loaded[row] = codes_of(bases), 1
            n[1] += 1
        else:
            seen.add(row)
            n[3] += 1
    return RefSeq(codes, loaded, Counters(*n))


def flat(ref, lengths):
    """-> bytes: what mg_refseq_download gives — the rows' codes back to back at the offsets of the lengths, 0xff in the rows
    that are not loaded."""
    return b''.join(ref.codes[r] if ref.loaded[r] else b'\xff' * int(L) for r, L in enumerate(lengths))


def read_bytes(path):
    """A reference file's bytes as they are parsed: a gzip / BGZF file (by its magic) inflated, every member."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:2] == b'\x1f\x8b':
        import gzip
        data = gzip.decompress(data)
    return data


assert OTHER == 4
