"""Test helper: reads built first, then written twice — as the FASTQ text they are, and as a BAM (tests/bamgen.py) holding the same
reads the way aligners and sequencers store them: unmapped records, mapped records on the reverse strand that store the reverse
complement, duplicate / QC-fail / paired flags, SEQ '*' for an empty read, and secondary / supplementary records with a DIFFERENT
SEQ mixed in, which a reads file must ignore (`samtools fastq -F 0x900`).  The expectation of every test is the FASTQ through the
existing path; nothing here uses metalign_amd/bam.py."""
import numpy as np

import bamgen
import util

# complement of every BAM letter (SAM specification §4.2.3 / htslib): A-T, C-G, M-K, R-Y, V-B, H-D; S, W, N, '=' stay
_COMP = str.maketrans("ACGTMKRYVBHDSWN=", "TGCAKMYRBVDHSWN=")
NAMES = ("g0", "g1", "g2")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def make_reads(seed=0, ntiles=40, nlong=3, k=21, long_range=(15000, 40000)):
    """The tile kinds of tests/util.py upper-cased (BAM stores neither lower case nor '.'), plus `nlong` reads of 15-40 kb.
    -> (list of str, genome bases, genome offsets)"""
    rng = np.random.default_rng(seed)
    gb, go = util.tile_genomes(rng, ngenomes=8, length=50000)
    kinds = util.tile_kinds(rng, ntiles)
    b, o = util.tile_sample(rng, gb, go, kinds, k)
    reads = [bytes(b[int(o[i]):int(o[i + 1])]).decode("latin-1").upper() for i in range(len(o) - 1)]
    for _ in range(nlong):
        g = int(rng.integers(0, len(go) - 1))
        n = int(rng.integers(long_range[0], long_range[1] + 1))
        a = int(go[g]) + int(rng.integers(0, int(go[g + 1] - go[g]) - n))
        s = bytes(gb[a:a + n]).decode("latin-1")
        at = int(rng.integers(len(reads) + 1))
        reads.insert(at, s if rng.random() < 0.5 else revcomp(s))
    return reads, gb, go


def fastq_text(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)).encode()


def sam_lines(reads, seed=1):
    """The SAM lines of a BAM that holds `reads` (in order) and records that are not reads."""
    rng = np.random.default_rng(seed)
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:60000" % n for n in NAMES]

    def line(q, flag, rname, cigar, seq, qual, tags=()):
        pos = "1" if rname != "*" else "0"
        return "\t".join([q, str(flag), rname, pos, "60" if rname != "*" else "0", cigar, "*", "0", "0", seq, qual] + list(tags))

    for i, s in enumerate(reads):
        q = "r%d" % i
        qual = "*" if rng.random() < 0.2 else "I" * len(s)
        extra = int(rng.choice([0, 0x400, 0x200, 0x1 | 0x40, 0x1 | 0x80])) if rng.random() < 0.3 else 0
        mode = rng.random()
        if not s:
            lines.append(line(q, 4 | extra, "*", "*", "*", "*"))
        elif mode < 0.35:  # unmapped, as the read is
            lines.append(line(q, 4 | extra, "*", "*", s, qual))
        elif mode < 0.45:  # unmapped with 0x10 set: stored reverse-complemented all the same
            lines.append(line(q, 4 | 0x10 | extra, "*", "*", revcomp(s), qual[::-1]))
        elif mode < 0.7:  # mapped, forward
            lines.append(line(q, extra, NAMES[i % 3], "%dM" % len(s), s, qual, ["NM:i:0"]))
        else:  # mapped, reverse strand: SEQ is the reverse complement
            lines.append(line(q, 0x10 | extra, NAMES[i % 3], "%dM" % len(s), revcomp(s), qual[::-1], ["NM:i:1"]))
        r = rng.random()
        if r < 0.15 and s:  # secondary / supplementary alignments of the same read, with a different SEQ (or none)
            n = int(rng.integers(1, 200))
            other = "".join(rng.choice(list("ACGT"), size=n))
            flag = int(rng.choice([0x100, 0x800, 0x900, 0x100 | 0x10, 0x800 | 0x10]))
            lines.append(line(q, flag, NAMES[(i + 1) % 3], "%dM" % n, other, "*"))
        elif r < 0.2:
            lines.append(line(q, 0x100, NAMES[i % 3], "10M", "*", "*"))  # SEQ '*' on a secondary
    return [ln + "\n" for ln in lines]


def bam_bytes(reads, seed=1, bgzf=True, block=65280):
    """-> (the BAM file's bytes, the record stream behind the header, n_ref)"""
    data, hdr, names = bamgen.encode(sam_lines(reads, seed))
    return (bamgen.bgzf(data, block=block) if bgzf else data), data[hdr:], len(names)


def bases_offsets(reads):
    """What the device parser leaves for the FASTQ of `reads`: (bases u8, offsets u64)."""
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in reads])
    b = np.frombuffer("".join(reads).encode("latin-1"), dtype=np.uint8) if reads else np.zeros(0, np.uint8)
    return b, offs
