"""Side outputs from uniquely assigned reads only (--side_reads unique): the definition, on the host.

By default every retained alignment that passes clean_read_hits' rule is painted onto its reference, whatever became of its read.
Under --side_reads unique coverage, depth and identity see only the alignments the profile itself counted as unique evidence for
their taxon.  A retained line L of read R survives when

    R's verdict (assignments.read_assignments over the same stream) is 'U', with taxid t;
    L is not the line the read loop drops: the first retained line of a read whose predecessor's verdict was 'A', and the first
        retained line of the file's first read (the phantom boundary);
    acc2info[RNAME of L][1] == t.

Lines of 'M', 'A' and 'N' reads never survive.  A surviving line may still fail a family's own counting rule (FLAG 2048, pct_id):
that rule is the family's, applied afterwards as it always is.  The three families in unique mode are then, by definition,

    coverage.coverage(unique_lines(lines, acc2info, pct_id), acc2info, pct_id)
    depth.depth(unique_lines(...), acc2info, pct_id, window)
    identity.identity(unique_lines(...), acc2info, pct_id)

Unlike the default side outputs these depend on how the lines are grouped into reads: a collated input is defined over
collate.collated_lines.

unique_mask_of_records states the same rule over tokenised records and stage C's verdict words; the device
(mg_records_mask_unique_dev, metalign_amd/csrc/mg_sidemask.hip) is held to it.
"""
import numpy as np

from . import _hip, assignments

HEADER_LINE = '#reads\tunique\n'  # behind a side file's column header in unique mode


def _is_header(line):
    if isinstance(line, (bytes, bytearray, memoryview)):
        return bytes(line[:1]) == b'@'
    return line.startswith('@')


def unique_lines(lines, acc2info, pct_id):
    """SAM lines (str or bytes) -> the header lines unchanged, and the retained lines that survive (the same objects), in order."""
    header = []

    def body():
        for line in lines:
            if _is_header(line):
                header.append(line)  # (handed on before anything that follows it)
            else:
                yield line

    for _, cls, taxids, _, mine in assignments._replay(body(), acc2info, pct_id):
        yield from header
        del header[:]
        if cls != 'U':
            continue
        for line, f, dropped in mine:
            if not dropped and acc2info[f[2]][1] == taxids[0]:
                yield line
    yield from header


def unique_mask_of_records(recs, words, ref2tax):
    """REC_DTYPE[n], the verdict words uint64[2 * reads] (the layout of mg_profile_commit_assign_dev: word 0 = kind | dense taxon
    << 2) and ref2tax (accession row -> dense taxon) -> bool[n], True where the record survives.  The ordinal of record i is the
    number of records in [0, i] with the new-read bit, minus one; a record is masked when that lies outside [0, reads), when its
    accession row is at or above len(ref2tax), when it is a new-read record of read 0 or of a read whose predecessor's kind is 0,
    when its read's kind is not 1, and when ref2tax[row] is not the read's taxon."""
    recs = np.ascontiguousarray(recs, dtype=_hip.REC_DTYPE)
    w0 = np.ascontiguousarray(words, dtype=np.uint64)[0::2]
    ref2tax = np.ascontiguousarray(ref2tax, dtype=np.uint32)
    nreads, nref = len(w0), len(ref2tax)
    new = (recs['ref_new'] & np.uint32(_hip.NEW_BIT)) != 0
    row = (recs['ref_new'] & np.uint32(_hip.REF_MASK)).astype(np.int64)
    ordinal = np.cumsum(new, dtype=np.int64) - 1
    ok = (ordinal >= 0) & (ordinal < nreads) & (row < nref)
    if not ok.any():
        return ok
    o = np.clip(ordinal, 0, nreads - 1)
    mine, before = w0[o], w0[np.clip(o - 1, 0, None)]
    dropped = new & ((ordinal == 0) | ((before & np.uint64(3)) == 0))
    taxon = ref2tax[np.clip(row, 0, nref - 1)].astype(np.uint64)
    return ok & ~dropped & ((mine & np.uint64(3)) == assignments.KIND_UNIQUE) & (taxon == (mine >> np.uint64(2)))


def outside_of_records(recs, words):
    """The records whose ordinal lies outside [0, reads): what mg_records_mask_unique_dev adds to d_stats2[1]."""
    recs = np.ascontiguousarray(recs, dtype=_hip.REC_DTYPE)
    ordinal = np.cumsum((recs['ref_new'] & np.uint32(_hip.NEW_BIT)) != 0, dtype=np.int64) - 1
    return int(np.count_nonzero((ordinal < 0) | (ordinal >= len(words) // 2)))
