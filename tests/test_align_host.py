"""CPU: metalign_amd/align.py (the seed-and-extend aligner's definition) against hand-worked cases, mg_align_core.h — the
per-position rules the kernels share — on the host under the sanitizers, the flags of --aligner device, and the planted-read
property on the definition alone."""
import os
import struct
import subprocess

import pytest

import align_cases as ac
from metalign_amd import align, map_and_profile, metalign, refseq
from metalign_amd.side_outputs import check_flags

HERE = os.path.dirname(os.path.abspath(__file__))

SEQ30 = b"ACGTTGCAAGGCTTACCGATNGGATCCATG"
# the keys of its ten k-mers without N (k = 11): fmix64 of the smaller of the k-mer's and its reverse complement's value
KEYS30 = [7234042558579858658, 13234970706070450598, 6685519133762789584, 6612064021808516018, 9196227227068807317,
          16816274296016258495, 15907139663978167982, 203459287016843992, 6464779334246926183, 1209901247457611011]


def value_of(kmer):
    return int(kmer.decode().translate(str.maketrans("ACGT", "0123")), 4)


def test_hand_keys_strand_bits_and_minimizers_of_30_bases():
    assert len(SEQ30) == 30 and SEQ30[20:21] == b"N"
    keys = align.kmer_keys(refseq.codes_of(SEQ30), 11)
    assert len(keys) == 20 and keys[10:] == [None] * 10  # every k-mer from position 10 on holds the N
    for p in range(10):
        kmer = SEQ30[p:p + 11]
        f, r = value_of(kmer), value_of(ac.revcomp(kmer))
        # (A < C < G < T as the codes: the values compare as the strings do)
        assert keys[p] == (align.fmix64(min(f, r)), 0 if kmer < ac.revcomp(kmer) else 1) and keys[p][0] == KEYS30[p]
    assert [s for _, s in keys[:10]] == [0, 0, 1, 1, 1, 0, 0, 0, 0, 1]
    # w = 5, m = 20: the windows [0, 5) .. [2, 7) choose 3, [3, 8) .. [7, 12) choose 7 (the smallest key of all), [8, 13) and
    # [9, 14) choose 9, the windows from 10 on hold no key
    assert align.minimizers(refseq.codes_of(SEQ30), 11, 5) == [(KEYS30[3], 3, 1), (KEYS30[7], 7, 0), (KEYS30[9], 9, 1)]
    assert [p for _, p, _ in align.minimizers(refseq.codes_of(SEQ30), 11, 1)] == list(range(10))  # w = 1: every keyed position
    assert align.minimizers(refseq.codes_of(SEQ30), 11, 32) == [(KEYS30[7], 7, 0)]  # m < w: one window of all positions
    assert align.minimizers(refseq.codes_of(SEQ30[:10]), 11, 5) == []  # m = 0: no window
    assert align.fmix64(0) == 0 and align.fmix64(1) == 0xb456bcfc34c2cb2c  # (MurmurHash3's finaliser)


def test_hand_equal_keys_the_leftmost_wins():
    # a period of 12 bases: positions 12 apart are the same k-mer, so every window of 13 k-mers holds its smallest key twice
    seq = b"ACGGTCATTGCA" * 4
    mins = align.minimizers(refseq.codes_of(seq), 11, 13)
    keys = align.kmer_keys(refseq.codes_of(seq), 11)
    assert keys[0] == keys[12] == keys[24]
    best = min(range(12), key=lambda q: keys[q][0])
    # window s holds positions s .. s + 12: the smallest key sits at best + 12 j; the first of them in the window wins
    want = sorted({min(q for q in range(s, s + 13) if q % 12 == best) for s in range(len(keys) - 13 + 1)})
    assert [p for _, p, _ in mins] == want and len(want) >= 2


def test_hand_candidates_of_one_read():
    p = align.params(k=11, w=5, max_occ=2)
    read = SEQ30  # L = 30, minimizers at 3 (strand 1), 7 (strand 0), 9 (strand 1)
    index = {
        KEYS30[3]: [(0, 100, 1)],                        # same strand bit: strand 0, d = 100 - 3
        KEYS30[7]: [(1, 50, 1), (1, 7, 0)],              # other bit: strand 1, d = 50 - (30 - 11 - 7); same: strand 0, d = 0
        KEYS30[9]: [(2, 5, 0), (2, 6, 0), (2, 7, 0)],    # three entries > max_occ = 2: seeds nothing
        KEYS30[0]: [(3, 1, 0)],                          # position 0 is no minimizer of the read
    }
    assert align.candidates(refseq.codes_of(read), index, p) == {(0, 0, 97), (1, 1, 38), (1, 0, 0)}
    index[KEYS30[7]].append((1, 9, 0))  # a second entry on the same diagonal as (1, 7, 0)? No: d = 9 - 7 = 2; three entries now
    assert align.candidates(refseq.codes_of(read), index, p) == {(0, 0, 97)}
    assert align.candidates(refseq.codes_of(read[:10]), index, p) == set()  # L < k
    assert align.candidates(refseq.codes_of(b"A" * 1025), {k: [(0, 0, 0)] for k in KEYS30}, p) == set()  # L > 1024
    # two minimizers on one diagonal are one candidate
    two = {KEYS30[3]: [(0, 103, 1)], KEYS30[7]: [(0, 107, 0)]}
    assert align.candidates(refseq.codes_of(read), two, p) == {(0, 0, 100)}


SCANS = [  # M adds 1, X subtracts P = 4, O lies outside the accession -> (score, b, e)
    ("", (0, 0, 0)),
    ("MMM", (3, 0, 3)),
    ("XMMM", (3, 1, 4)),
    ("XXXX", (0, 0, 0)),
    ("MMMXMMMM", (4, 4, 8)),       # 3, then the X resets (3 - 4 <= 0), then 4 > 3
    ("MMMXMMM", (3, 0, 3)),        # a tie: the first segment to reach 3 keeps it
    ("MMMMMXMM", (5, 0, 5)),       # 5, 1, 2, 3: never above 5 again
    ("MMMMMMXMMMMM", (7, 0, 12)),  # 6, 2, then 3 .. 7: one segment with one mismatch
    ("OOMMM", (3, 2, 5)),          # an outside run in front
    ("MMOMMM", (3, 3, 6)),         # an outside column resets like a new start
    ("MMOMM", (2, 0, 2)),          # ... and a tie across it goes to the first
    ("MMMOO", (3, 0, 3)),
    ("XXMMMM", (4, 2, 6)),         # a segment that ends on the last column
    ("MMMMXMMMMX", (4, 0, 4)),     # 4, 0 (4 - 4 <= 0 resets), 4: a tie again
]


def cols_of(pattern):
    return [None if c == "O" else c == "M" for c in pattern]


@pytest.mark.parametrize("pattern,want", SCANS)
def test_hand_scan_patterns(pattern, want):
    assert align.scan(cols_of(pattern), 4) == want


def test_hand_extension_on_a_reference():
    ref = refseq.codes_of(b"ACGTACGTNACGT")
    # d = -2: two columns outside; ref ACGTAC.. against GGACGTAC: match from column 2 on
    assert align.extend(refseq.codes_of(b"GGACGTAC"), ref, -2, 4) == (6, 2, 8, 0)
    # the N of the reference matches nothing, not even an N of the read: ACGTNACGT scores 4, 0, 4 -> the first 4
    assert align.extend(refseq.codes_of(b"ACGTNACGT"), ref, 4, 4) == (4, 0, 4, 0)
    # hanging over the right end: columns 3 .. 5 lie outside
    assert align.extend(refseq.codes_of(b"CGTAAA"), ref, 10, 4) == (3, 0, 3, 0)
    # one mismatch inside a long segment is counted by nm
    assert align.extend(refseq.codes_of(b"ACGTACCTN"), refseq.codes_of(b"ACGTACGTNACGT"), 0, 1) == (6, 0, 6, 0)
    assert align.extend(refseq.codes_of(b"ACGTAGGTAC"), refseq.codes_of(b"ACGTACGTAC"), 0, 1) == (8, 0, 10, 1)


def A(a, strand, pos0, span, score):
    return align.Aln(a, strand, pos0, score, 0, span, 0)  # (b = 0: d = pos0)


def test_hand_selection_rules():
    p = align.params(max_secondary=2, sec_pct=80)
    al = [A(0, 0, 100, 50, 50), A(0, 0, 120, 50, 50), A(0, 1, 120, 50, 48), A(1, 0, 100, 50, 45), A(0, 0, 150, 40, 40), A(2, 0, 0, 39, 39)]
    # (0, 0, 120) overlaps the primary on the same row and strand; the other strand and the other row do not; two secondaries fill it
    assert align.select(al, p) == [al[0], al[2], al[3]]
    # intervals that touch do not intersect: [100, 150) and [150, 190)
    assert align.select(al, align.params(max_secondary=5, sec_pct=80)) == [al[0], al[2], al[3], al[4]]  # 39 * 100 < 50 * 80
    assert align.select(al, align.params(max_secondary=5, sec_pct=78)) == [al[0], al[2], al[3], al[4], al[5]]
    assert align.select(al, align.params(max_secondary=0)) == [al[0]]
    # the order: score descending, then a, pos0, strand, d
    tie = [align.Aln(1, 0, 5, 40, 0, 40, 0), align.Aln(0, 1, 9, 40, 0, 40, 0), align.Aln(0, 0, 9, 40, 0, 40, 0),
           align.Aln(0, 0, 3, 40, 6, 46, 0), align.Aln(0, 0, 500, 41, 0, 41, 0)]
    # (0, 0, d = 3, b = 6) and (0, 0, d = 9, b = 0) both start at pos0 = 9 on strand 0: d = 3 first, and they overlap
    assert align.select(tie, align.params(max_secondary=5, sec_pct=0)) == [tie[4], tie[3], tie[1], tie[0]]
    assert align.select([], p) == []


def test_hand_sam_lines_byte_for_byte():
    names, lengths = ["accA", "accB"], [1000, 77]
    reads = [b"ACGTNacgtAC", b"GGGGCCCCAA", b"TTTT"]
    headers = [b"r1 first/1", b"r2\tx", b"r3"]
    quals = [b"ABCDEFGHIJK", b"0123456789", b"!!!!"]
    alns = [[align.Aln(0, 0, 99, 8, 1, 10, 1), align.Aln(1, 1, -2, 7, 2, 11, 2)],
            [align.Aln(1, 1, 5, 10, 0, 10, 0)],
            []]
    want = (b"@SQ\tSN:accA\tLN:1000\n@SQ\tSN:accB\tLN:77\n"
            b"r1\t0\taccA\t101\t255\t1S9M1S\t*\t0\t0\tACGTNacgtAC\tABCDEFGHIJK\tNM:i:1\n"
            b"r1\t272\taccB\t1\t255\t2S9M\t*\t0\t0\t*\t*\tNM:i:2\n"
            b"r2\t16\taccB\t6\t255\t10M\t*\t0\t0\tTTGGGGCCCC\t9876543210\tNM:i:0\n")
    assert b"".join(align.sam_lines(headers, reads, quals, names, lengths, alns)) == want
    # without qualities (FASTA reads): `*`; a byte that is no base becomes N
    got = align.sam_lines([b"q"], [b"AC-RT"], None, names, lengths, [[align.Aln(0, 1, 0, 5, 0, 5, 0)]])
    assert got[-1] == b"q\t16\taccA\t1\t255\t5M\t*\t0\t0\tANNGT\t*\tNM:i:0\n"


def test_records_of_the_definition():
    reads = [b"ACGTNacgtAC", b"TTTT"]
    alns = [[align.Aln(0, 0, 99, 8, 1, 10, 1), align.Aln(1, 1, -2, 7, 2, 11, 2)], []]
    recs, places, edits, entries, pool = align.records(reads, alns)
    assert recs.tolist() == [(0x80000000, 9, 11, 11 << 12), (1, 9, 11, 256 + 16)]
    assert places.tolist() == [(100, 9), (0, 9)] and edits.tolist() == [(1, 9), (2, 9)]
    assert entries.tolist() == [(0, 100, 9), (0, 0, 0)]  # a secondary is not piled: its SEQ is `*`
    assert pool == bytes([1 | 2 << 4, 3 | 4 << 4, 0 | 1 << 4, 2 | 3 << 4, 0])  # CGTNacgtA, two codes per byte, the low nibble first


def test_parameter_ranges():
    assert align.params() == (15, 5, 64, 30, 4, 5, 80)
    for bad in (dict(k=10), dict(k=9), dict(k=33), dict(k=16), dict(w=0), dict(w=33), dict(max_occ=0), dict(min_score=0),
                dict(min_score=1025), dict(mismatch=0), dict(mismatch=65), dict(max_secondary=-1), dict(max_secondary=16),
                dict(sec_pct=-1), dict(sec_pct=101)):
        with pytest.raises(ValueError):
            align.params(**bad)
    for k, w in ac.PARAMS:
        align.params(k=k, w=w)


# ---- the flags ------------------------------------------------------------------------------------------------------------------
def test_flags_parse_with_their_defaults():
    for parse, argv in ((map_and_profile.profile_parseargs, ["reads.fq", "data"]), (metalign.metalign_parseargs, ["reads.fq", "data"])):
        a = parse(argv)
        assert (a.aligner, a.align_k, a.align_w, a.align_max_occ, a.align_min_score, a.align_mismatch, a.align_secondary,
                a.align_secondary_pct) == ("minimap2", 15, 5, 64, 30, 4, 5, 80)
        a = parse(argv + ["--aligner", "device", "--align_k", "21", "--align_w", "9", "--align_max_occ", "8", "--align_min_score", "40",
                          "--align_mismatch", "3", "--align_secondary", "2", "--align_secondary_pct", "90"])
        assert (a.aligner, a.align_k, a.align_w, a.align_max_occ, a.align_min_score, a.align_mismatch, a.align_secondary,
                a.align_secondary_pct) == ("device", 21, 9, 8, 40, 3, 2, 90)
        check_flags(a)
        with pytest.raises(SystemExit):
            parse(argv + ["--aligner", "bwa"])


REFUSED = [
    (["--read_assignments", "rows.tsv"], "--read_assignments"),
    (["--collate", "auto"], "--collate"),
    (["--collate", "always"], "--collate"),
    (["--align_k", "16"], "--align_k"),
    (["--align_k", "9"], "--align_k"),
    (["--align_k", "33"], "--align_k"),
    (["--align_w", "0"], "--align_w"),
    (["--align_w", "33"], "--align_w"),
    (["--align_max_occ", "0"], "--align_max_occ"),
    (["--align_min_score", "0"], "--align_min_score"),
    (["--align_min_score", "2000"], "--align_min_score"),
    (["--align_mismatch", "0"], "--align_mismatch"),
    (["--align_secondary", "-1"], "--align_secondary"),
    (["--align_secondary", "16"], "--align_secondary"),
    (["--align_secondary_pct", "101"], "--align_secondary_pct"),
]


@pytest.mark.parametrize("extra,named", REFUSED)
@pytest.mark.parametrize("tool", ["map_and_profile", "metalign"])
def test_check_flags_refuses(tool, extra, named):
    parse = map_and_profile.profile_parseargs if tool == "map_and_profile" else metalign.metalign_parseargs
    argv = ["reads.fq", "data", "--aligner", "device"] + (["--db", "db.fna"] if tool == "map_and_profile" else []) + extra
    with pytest.raises(SystemExit) as e:
        check_flags(parse(argv))
    assert str(e.value).startswith("Error: ") and named in str(e.value)
    # without --aligner device none of them is refused on the aligner's account
    quiet = [x for x in argv if x not in ("--aligner", "device")]
    if extra[0] not in ("--read_assignments", "--collate"):
        check_flags(parse(quiet))


def test_the_flag_is_a_no_op_for_alignment_files():
    for name in ("x.sam", "x.bam", "x.paf"):
        a = map_and_profile.profile_parseargs([name, "data", "--aligner", "device", "--collate", "auto", "--align_k", "16"])
        check_flags(a)
    a = map_and_profile.profile_parseargs(["x.txt", "data", "--input_type", "sam", "--aligner", "device", "--collate", "always"])
    check_flags(a)


# ---- mg_align_core.h on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("align") / "host_align_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", out, os.path.join(HERE, "host_align_check.cpp")])
    return out


def run_check(exe, tmp_path, seqs, scans, sels):
    """seqs: (k, w, codes); scans: (P, columns as align.columns gives them); sels: (max_secondary, sec_pct, [Aln] in order) ->
    the program's ([minimizers (key, p, s)], [(score, b, e, nm)], [kept indices])."""
    blob = [struct.pack("<I", len(seqs))]
    for k, w, codes in seqs:
        blob.append(struct.pack("<III", k, w, len(codes)) + bytes(codes))
    blob.append(struct.pack("<I", len(scans)))
    for P, cols in scans:
        blob.append(struct.pack("<II", P, len(cols)) + bytes(0 if c is None else 1 if c else 2 for c in cols))
    blob.append(struct.pack("<I", len(sels)))
    for ms, pct, alns in sels:
        blob.append(struct.pack("<III", ms, pct, len(alns)))
        blob += [struct.pack("<5I", al.a, al.strand, al.d + al.b, al.e - al.b, al.score) for al in alns]
    p = tmp_path / "cases.bin"
    p.write_bytes(b"".join(blob))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "%d sequences, %d scans, %d selections" % (len(seqs), len(scans), len(sels))
    mins, got_scans, got_sels = [], [], []
    for ln in lines[:-1]:
        f = ln.split()
        if f[0] == "S":
            mins.append([])
        elif f[0] == "m":
            mins[-1].append((int(f[2]), int(f[1]), int(f[3])))
        elif f[0] == "C":
            got_scans.append(tuple(int(x) for x in f[2:]))
        elif f[0] == "K":
            got_sels.append([int(x) for x in f[2:]])
    return mins, got_scans, got_sels


def test_core_header_on_the_hand_cases(exe, tmp_path):
    codes = refseq.codes_of(SEQ30)
    seqs = [(11, w, codes[:n]) for w in (1, 2, 5, 13, 32) for n in (0, 10, 11, 12, 15, 30)]
    seqs.append((11, 13, refseq.codes_of(b"ACGGTCATTGCA" * 4)))
    scans = [(4, cols_of(pattern)) for pattern, _ in SCANS]
    mins, got, _ = run_check(exe, tmp_path, seqs, scans, [])
    assert mins == [align.minimizers(c, k, w) for k, w, c in seqs]
    assert [g[:3] for g in got] == [want for _, want in SCANS]


@pytest.mark.parametrize("k,w", ac.PARAMS)
def test_core_header_against_the_definition_over_the_generators(exe, tmp_path, k, w):
    t = ac.table(k, w)
    seqs = [(k, w, t.ref.codes[a]) for a in sorted(t.ref.codes)]
    seqs += [(k, w, refseq.codes_of(s)) for _, s in t.reads] + [(k, w, align.revcomp_codes(refseq.codes_of(s))) for _, s in t.reads]
    scans, want_scans, sels, want_sels = [], [], [], []
    for _, seq in t.reads:
        codes = refseq.codes_of(seq)
        rc, accepted = align.revcomp_codes(codes), []
        for a, strand, d in sorted(align.candidates(codes, t.index, t.p)):
            o = rc if strand else codes
            scans.append((t.p.mismatch, align.columns(o, t.ref.codes[a], d)))
            want_scans.append(align.extend(o, t.ref.codes[a], d, t.p.mismatch))
            if want_scans[-1][0] >= t.p.min_score:
                accepted.append(align.Aln(a, strand, d, *want_scans[-1]))
        if accepted:
            accepted.sort(key=align.order_key)
            for ms, pct in ((t.p.max_secondary, t.p.sec_pct), (0, 80), (15, 0)):
                sels.append((ms, pct, accepted))
                kept = align.select(accepted, t.p._replace(max_secondary=ms, sec_pct=pct))
                want_sels.append([accepted.index(x) for x in kept])
    assert len(scans) > 50 and len(sels) > 60
    mins, got_scans, got_sels = run_check(exe, tmp_path, seqs, scans, sels)
    assert mins == [align.minimizers(c, k, w) for _, _, c in seqs]
    assert got_scans == want_scans and got_sels == want_sels


# ---- the planted-read property ------------------------------------------------------------------------------------------------
def test_planted_reads_are_found_at_five_percent_substitutions():
    """3 random genomes of 20 000 bases, 300 reads of 150, every base substituted with probability 0.05, half of them
    reverse-complemented, every parameter at its default: at least 98 % of the primaries at the true (accession, strand, diagonal)."""
    names, lengths, fasta, ref, reads, truth = ac.property_inputs()
    assert len(reads) == 300 and sum(1 for _, s, _ in truth if s) == 150 and lengths == [20000] * 3
    alns, stats = align.align_reads([s for _, s in reads], ref, align.params())
    right = sum(1 for kept, tr in zip(alns, truth) if kept and (kept[0].a, kept[0].strand, kept[0].d) == tr)
    print("primary at the true place: %d of %d; %s" % (right, len(reads), stats))
    assert right * 100 >= 98 * len(reads)
