"""Per-read taxon assignments of stage C (--read_assignments): the definition, on the host.

What the profile sums up, read by read.  The loop of the reference (scripts/map_and_profile.py:193-264, process_read
:152-176) decides a read's fate when the first retained line of the NEXT read arrives: that line's pair flags are what
process_read is told (:225-226), an Ambiguous verdict makes the loop skip that line (:229-232: the next read loses its first
line), the loop's very first boundary is a phantom read without lines (Ambiguous, so the file's first read loses its first
line too) and the file's last read is never decided at all (:259-264).  read_assignments replays exactly that and yields,
per read and in file order,

    (qname, cls, taxids, hit_bases)

    cls 'U'  unique        taxids = [the taxid]                                   hit_bases = hitlen
        'M'  multimapped   taxids = what the reference appends at :246, in order  hit_bases = hitlen
        'A'  ambiguous     taxids = []                                            hit_bases = -1
        'N'  not counted   taxids = []   (the file's last read)                   hit_bases = -1

so that: rows = tot_rds; 'A' rows + 1 (the phantom) = the Unmapped count; 'U' rows fold into taxids2abs' counts and bases in
order of first appearance; 'M' rows are `multimapped`.  hit_bases is the raw integer whatever --length_normalize says.

The device path (mg_profile_commit_assign_dev + the named tokenisers, metalign_amd/_hip.py) is checked against this file.
"""

HEADER = '#read\tclass\ttaxids\thit_bases\n'


def _fields_of(line):
    """The fields of a retained line (:206-213), None for every other line."""
    if isinstance(line, (bytes, bytearray, memoryview)):
        line = bytes(line).decode('utf-8')
    if line.startswith('@'):
        return None
    f = line.strip().split()
    if len(f) < 6:
        return None
    if (int(f[1]) & 4) or f[5] == '*':
        return None
    return f


def _fails_pct_id(f, pct_id):
    """filter_line (:86-100), with everything it raises."""
    matched = total = cur = 0
    for ch in f[5]:
        if ch.isalpha():
            if ch == 'M' or ch == '=':
                matched += cur
            total += cur
            cur = 0
        else:
            cur = cur * 10 + int(ch)
    int(f[11][5:])
    return float(matched) / float(total) < pct_id


def _decide(hits, next_pair1, next_pair2, pct_id):
    """process_read (:152-176) over a read's lines [(fields, taxid)] -> (cls, taxids, hit_bases)."""
    ends1 = ends2 = 0  # (:257-258, summed while the lines came in)
    for f, _ in hits:
        flag = int(f[1])
        p1, p2 = bool(flag & 1 and flag & 64), bool(flag & 1 and flag & 128)
        ends1 += p1 or not (p1 or p2)
        ends2 += p2
    kept, hitlen = [], 0
    for f, taxid in hits:  # clean_read_hits (:130-147)
        flag = int(f[1])
        if _fails_pct_id(f, pct_id) or flag & 2048:
            if flag & 1 and flag & 64:
                ends1 -= 1
            elif flag & 1 and flag & 128:
                ends2 -= 1
        else:
            kept.append(taxid)
        if f[9] != '*':
            hitlen += len(f[9])
    if not kept:
        return 'A', [], -1  # :156
    if next_pair1 or next_pair2:
        if ends1 + ends2 == 1:
            return 'U', [kept[0]], hitlen  # :160
        if ends1 == 0 or ends2 == 0:
            return 'A', [], -1  # :165 (intersect_read_hits :116-117)
        second = kept[ends1:]
        both = set(t for t in kept[:ends1] if t in second)
        if not both:
            return 'A', [], -1  # :165
        if len(both) == 1:
            return 'U', [kept[0]], hitlen  # :167
        return 'M', [t for t in kept if t in both], hitlen  # :169
    if ends1 > 1:
        return 'M', kept, hitlen  # :173
    return 'U', [kept[0]], hitlen  # :176


def _replay(lines, acc2info, pct_id):
    """The loop itself: per read and in file order (qname, cls, taxids, hit_bases, its retained lines [(line, fields, dropped)]),
    dropped = the line the loop never counts in (:232).  read_assignments and side_reads.unique_lines are both this replay."""
    prev, hits, opened, mine = '', [], False, []
    for line in lines:
        f = _fields_of(line)
        if f is None:
            continue
        taxid = acc2info[f[2]][1]
        if f[0] != prev:
            flag = int(f[1])
            if opened:
                verdict = _decide(hits, bool(flag & 1 and flag & 64), bool(flag & 1 and flag & 128), pct_id)
                yield (prev,) + verdict + (mine,)
                dropped = verdict[0] == 'A'
            else:
                dropped = True  # the phantom first boundary: a read without lines is Ambiguous (:155-156)
            prev, hits, opened, mine = f[0], [], True, []
            if dropped:
                mine.append((line, f, True))
                continue  # (:232: this line is never counted in)
        hits.append((f, taxid))
        mine.append((line, f, False))
    if opened:
        yield prev, 'N', [], -1, mine


def read_assignments(lines, acc2info, pct_id):
    """SAM lines (str or bytes) -> one (qname, cls, taxids, hit_bases) per read, in file order."""
    for row in _replay(lines, acc2info, pct_id):
        yield row[:4]


def fold(rows):
    """The rows summed up as the reference sums them: (unique {taxid: [reads, bases]} in order of first appearance, the Unmapped
    count, tot_rds, the multimapped lists [taxid, ..., hitlen])."""
    unique, ambiguous, total, multimapped = {}, 1, 0, []
    for _, cls, taxids, hit_bases in rows:
        total += 1
        if cls == 'U':
            ent = unique.setdefault(taxids[0], [0, 0])
            ent[0] += 1
            ent[1] += hit_bases
        elif cls == 'M':
            multimapped.append(list(taxids) + [hit_bases])
        elif cls == 'A':
            ambiguous += 1
    if total == 0:
        ambiguous = 0  # (no line, no boundary: not even the phantom)
    return unique, ambiguous, total, multimapped


def format_row(row):
    qname, cls, taxids, hit_bases = row
    return '%s\t%s\t%s\t%d\n' % (qname, cls, ','.join(taxids) if taxids else '-', hit_bases)


def write_assignments(path, rows, append=False):
    """TSV: the header line (a new file only), then one line per read; taxids comma-joined, '-' for none."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER)
        for row in rows:
            out.write(format_row(row))


# ---- the device's words -> the same rows ------------------------------------------------------------------------------
KIND_AMBIGUOUS, KIND_UNIQUE, KIND_MULTI, KIND_NOT_COUNTED = 0, 1, 2, 3
_CLS = 'AUMN'


def rows_from_words(words, names, name_off, taxids, mm_offsets, mm_tax, mm_hitlen):
    """mg_profile_commit_assign_dev's words (uint64[2 * reads]: kind | dense taxon << 2, hitlen or multimapped CSR row), the reads'
    QNAMEs (bytes + uint64 offsets) and the multimapped CSR -> the rows read_assignments gives."""
    nreads = len(words) // 2
    if len(name_off) != nreads + 1:
        raise ValueError('%d names for %d reads' % (len(name_off) - 1, nreads))
    blob = bytes(names)
    for r in range(nreads):
        w0, w1 = int(words[2 * r]), int(words[2 * r + 1])
        kind = w0 & 3
        qname = blob[int(name_off[r]):int(name_off[r + 1])].decode('utf-8')
        if kind == KIND_UNIQUE:
            yield qname, 'U', [taxids[w0 >> 2]], w1
        elif kind == KIND_MULTI:
            row = [taxids[int(t)] for t in mm_tax[int(mm_offsets[w1]):int(mm_offsets[w1 + 1])]]
            yield qname, 'M', row, int(mm_hitlen[w1])
        else:
            yield qname, _CLS[kind], [], -1
