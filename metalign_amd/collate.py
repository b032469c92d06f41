"""Collating alignments by read: the DEFINITION the device is held to (metalign_amd/csrc/mg_collate.hip), and the fallback
whenever the device path declines a file.  Pure Python.

Stage C assumes that all alignments of a read sit next to each other: the reference's loop closes a read when `read != prev_read`
(/root/reference/scripts/map_and_profile.py:201-259).  An aligner writes them that way; `samtools sort` orders by coordinate by
default and scatters them.  collated_lines puts them back together:

  * the header lines ('@') come first, unchanged and in their order;
  * only RETAINED alignment lines follow — the rule of :206-213: not '@', at least 6 fields, FLAG without 4, CIGAR not '*'.  The
    others are dropped: stage C ignores them anyway;
  * a group is the retained lines of one QNAME; the groups come in the order of their FIRST retained line in the file;
  * inside a group the lines are sorted by (mate-2 class, not primary, file index).  Mate-2 class is `flag & 1 and flag & 128 and
    not flag & 64` — the reference's `pair2 and not pair1`: intersect_read_hits slices [:pair1maps], so read-1 lines must come
    first.  Not primary is `flag & 0x900` (secondary or supplementary).

A name-grouped aligner output (read-1 primary, its secondaries, read-2 primary, its secondaries) is a fixed point of this order.

THE RESULT DEPENDS ON THE ORDER OF THE GROUPS, because the reference's loop does:

  * it takes the pairing flags that decide a read from the NEXT read's first line (:225-226);
  * an Ambiguous read drops the next read's first line (:229-232);
  * the last read is never flushed.

So the profile of a collated file is the reference's profile OF THE COLLATED TEXT — not the profile of whatever name-grouped file
the input was once sorted from (single and paired reads interleave differently after collation, and most taxa move a little).
Expected values therefore always come from collated_lines of the file at hand.
"""


def _text(line):
    return line.decode('utf-8') if isinstance(line, (bytes, bytearray)) else line


def _retained(line):
    """(QNAME, FLAG) of a retained line, None for any other (:204-213).  int(FLAG) raises what the reference raises."""
    if line.startswith('@'):
        return None
    f = line.strip().split()
    if len(f) < 6:
        return None
    flag = int(f[1])
    if (flag & 4) or f[5] == '*':
        return None
    return f[0], flag


def sort_key(flag, index):
    """A retained line's place inside its read."""
    mate2 = 1 if (flag & 1) and (flag & 128) and not (flag & 64) else 0
    return mate2, 1 if flag & 0x900 else 0, index


def collated_lines(lines):
    """SAM lines (str or bytes) -> the header lines, then the retained alignment lines in collated order (the same objects)."""
    header, groups = [], {}
    for i, raw in enumerate(lines):
        line = _text(raw)
        if line.startswith('@'):
            header.append(raw)
            continue
        got = _retained(line)
        if got is None:
            continue
        groups.setdefault(got[0], []).append((sort_key(got[1], i), raw))
    out = header
    for members in groups.values():  # (a dict keeps the order of first insertion)
        members.sort(key=lambda m: m[0])
        out.extend(raw for _, raw in members)
    return out


def header_says_coordinate(header_lines):
    """True when an @HD line carries SO:coordinate (what `--collate auto` looks at)."""
    for ln in header_lines:
        ln = _text(ln)
        if ln.startswith('@HD') and 'SO:coordinate' in ln.rstrip('\r\n').split('\t'):
            return True
    return False
