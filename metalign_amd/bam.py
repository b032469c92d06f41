"""BAM files on the host: detection, the header, the SAM rendering of every record (SAM specification §4.2, as
`samtools view -h` prints it), and the FASTQ rendering of a BAM READS file (fastq_records, as `samtools fastq` writes it).

The device decodes BAM records itself (metalign_amd/csrc/mg_bam.hip); this module is the DEFINITION it is held to.  A record
the device does not decide, or a file it refuses, is rendered here line by line and fed to the SAM path (map_and_process),
which raises what the reference raises on that line.  Pure Python: zlib (through gzip) and struct.
"""
import gzip
import struct
import sys
import zlib

MAGIC = b"BAM\x01"
# the BGZF end-of-file marker: an empty block (SAM specification §4.1.2)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"
_AUX_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_B_SUB = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def _is_gzip(path):
    with open(path, "rb") as fh:
        return fh.read(2) == b"\x1f\x8b"


def is_bam(path):
    """True when the file starts with the BAM magic — as it is, or once its first gzip (BGZF) member is inflated."""
    try:
        with open(path, "rb") as fh:
            head = fh.read(1 << 16)
    except OSError:
        return False
    if head[:2] != b"\x1f\x8b":
        return head[:4] == MAGIC
    try:
        return zlib.decompressobj(31).decompress(head, 4)[:4] == MAGIC
    except zlib.error:
        return False


def has_eof_block(path):
    with open(path, "rb") as fh:
        fh.seek(0, 2)
        if fh.tell() < len(BGZF_EOF):
            return False
        fh.seek(-len(BGZF_EOF), 2)
        return fh.read() == BGZF_EOF


class BamReader:
    """The header (text, reference names) on opening; records() -> the raw record bodies (without block_size), in file order.
    A truncated or corrupt file raises ValueError naming it."""

    def __init__(self, path):
        self.path = path
        self.fh = gzip.open(path, "rb") if _is_gzip(path) else open(path, "rb")
        try:
            if self._read(4) != MAGIC:
                raise ValueError("%s: not a BAM file" % path)
            (l_text,) = struct.unpack("<i", self._read(4))
            self.text = self._read(l_text).split(b"\0", 1)[0].decode("utf-8", "replace")
            (n_ref,) = struct.unpack("<i", self._read(4))
            self.names = []
            for _ in range(n_ref):
                (l_name,) = struct.unpack("<i", self._read(4))
                self.names.append(self._read(l_name).split(b"\0", 1)[0])
                self._read(4)
        except (ValueError, struct.error):
            self.fh.close()
            raise
        except (OSError, EOFError, zlib.error) as e:
            self.fh.close()
            raise ValueError("%s: unreadable BAM header (%s)" % (path, e)) from e

    def _read(self, n, eof_ok=False):
        try:
            b = self.fh.read(n)
        except (OSError, EOFError, zlib.error) as e:
            raise ValueError("%s: corrupt or truncated BAM file (%s)" % (self.path, e)) from e
        if len(b) != n and not (eof_ok and not b):
            raise ValueError("%s: truncated BAM file (a record runs past the end)" % self.path)
        return b

    def records(self):
        n_ref = len(self.names)
        i = 0
        try:
            while True:
                head = self._read(4, eof_ok=True)
                if not head:
                    return
                (bs,) = struct.unpack("<I", head)
                if bs < 33:
                    raise ValueError("%s: corrupt BAM record %d (block_size %d)" % (self.path, i, bs))
                body = self._read(bs)
                ref, _, l_rn, _, _, ncig, _, l_seq, nref = struct.unpack_from("<iiBBHHHIi", body, 0)
                if (not (-1 <= ref < n_ref and -1 <= nref < n_ref) or l_rn < 1
                        or 32 + l_rn + 4 * ncig + (l_seq + 1) // 2 + l_seq > bs or body[32 + l_rn - 1] != 0):
                    raise ValueError("%s: corrupt BAM record %d" % (self.path, i))
                yield body
                i += 1
        finally:
            self.fh.close()


def _aux(body, p, end, path):
    """-> (rendered field, next offset)"""
    tag = body[p:p + 2].decode("latin-1")
    ty = chr(body[p + 2])
    p += 3
    if ty == "A":
        return "%s:A:%s" % (tag, chr(body[p])), p + 1
    if ty in _AUX_INT:
        fmt = _AUX_INT[ty]
        return "%s:i:%d" % (tag, struct.unpack_from(fmt, body, p)[0]), p + struct.calcsize(fmt)
    if ty == "f":
        return "%s:f:%g" % (tag, struct.unpack_from("<f", body, p)[0]), p + 4
    if ty in "ZH":
        e = body.index(b"\0", p, end)
        return "%s:%s:%s" % (tag, ty, body[p:e].decode("latin-1")), e + 1
    if ty == "B":
        sub = chr(body[p])
        (cnt,) = struct.unpack_from("<I", body, p + 1)
        fmt = _B_SUB.get(sub)
        if fmt is None:
            raise ValueError("%s: corrupt BAM aux field %s" % (path, tag))
        sz = struct.calcsize(fmt)
        vals = [struct.unpack_from(fmt, body, p + 5 + k * sz)[0] for k in range(cnt)]
        txt = "".join((",%g" % v) if sub == "f" else (",%d" % v) for v in vals)
        return "%s:B:%s%s" % (tag, sub, txt), p + 5 + cnt * sz
    raise ValueError("%s: corrupt BAM aux field %s (type %r)" % (path, tag, ty))


def render(body, names, path="BAM"):
    """One record body -> its SAM line (bytes, with the newline), as samtools prints it."""
    ref, pos, l_rn, mapq, _, ncig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHIiii", body, 0)
    p = 32
    qname = body[p:p + l_rn - 1].decode("latin-1")
    p += l_rn
    ops = struct.unpack_from("<%dI" % ncig, body, p) if ncig else ()
    p += 4 * ncig
    if any((v & 15) > 8 for v in ops):
        raise ValueError("%s: corrupt BAM record %s (CIGAR op above 8)" % (path, qname))
    cigar = "".join("%d%s" % (v >> 4, CIGAR_OPS[v & 15]) for v in ops) if ops else "*"
    packed = body[p:p + (l_seq + 1) // 2]
    p += (l_seq + 1) // 2
    seq = "".join(SEQ_CODES[(packed[k >> 1] >> (4 * (1 - (k & 1)))) & 15] for k in range(l_seq)) if l_seq else "*"
    qual = body[p:p + l_seq]
    p += l_seq
    qual = "*" if (not l_seq or qual[0] == 0xFF) else "".join(chr((q + 33) & 0xFF) for q in qual)
    tags = []
    end = len(body)
    while p < end:
        t, p = _aux(body, p, end, path)
        tags.append(t)
    if (not (flag & 4) and ncig == 2 and (ops[0] & 15) == 4 and (ops[0] >> 4) == l_seq and (ops[1] & 15) == 3
            and any(t.startswith("CG:") for t in tags)):
        raise ValueError("%s: read %s keeps its CIGAR in a CG tag (long-read BAM): not supported" % (path, qname))
    rname = names[ref].decode("latin-1") if ref >= 0 else "*"
    rnext = "*" if nref < 0 else ("=" if nref == ref else names[nref].decode("latin-1"))
    fields = [qname, str(flag), rname, str(pos + 1), str(mapq), cigar, rnext, str(npos + 1), str(tlen), seq, qual] + tags
    return ("\t".join(fields) + "\n").encode("latin-1")


def sam_lines(path):
    """The file's SAM rendering, line by line (bytes): the header text, then one line per record."""
    rd = BamReader(path)
    for ln in rd.text.splitlines(True):
        yield ln.encode("utf-8")
    for body in rd.records():
        yield render(body, rd.names, path)


_SEQ_PAIRS = [(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15]).encode() for b in range(256)]
_SEQ_COMP = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")
NOT_READ = 0x900  # secondary (0x100) | supplementary (0x800): not a read (`samtools fastq`'s default -F 0x900)
ABSENT_QUAL = 1   # the quality written for a record without QUAL (0xff)


def fastq_records(path):
    """A BAM READS file -> its FASTQ rendering, one record (bytes, four lines) at a time, as `samtools fastq` with its default filter
    writes it: every record that is neither secondary (0x100) nor supplementary (0x800), in file order; the name is QNAME; SEQ
    decoded through "=ACMGRSVTWYHKDBN" and, for 0x10, reverse-complemented back to the read's own orientation (A<->T, C<->G, M<->K,
    R<->Y, V<->B, H<->D; S, W, N, '=' kept); QUAL + 33, reversed for 0x10.  A record without QUAL (0xff) gets quality 1 ('"') at
    every base: believed to be `samtools fastq -v 1`'s default, not checked against samtools here.  SEQ '*' is an empty read.
    The device path (mg_reads_parse_bam_prefix_dev) uses the same rules for the bases; it is held to the FASTQ the reads came from,
    not to this function.  A truncated or corrupt file raises ValueError naming it."""
    rd = BamReader(path)
    for body in rd.records():
        l_rn, ncig, flag, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<H", body, 14)[0], \
            struct.unpack_from("<I", body, 16)[0]
        if flag & NOT_READ:
            continue
        name = body[32:32 + l_rn - 1]
        p = 32 + l_rn + 4 * ncig
        packed = body[p:p + (l_seq + 1) // 2]
        seq = b"".join(_SEQ_PAIRS[b] for b in packed)[:l_seq]
        qual = body[p + (l_seq + 1) // 2:p + (l_seq + 1) // 2 + l_seq]
        if l_seq and qual[0] == 0xFF:
            qual = bytes([ABSENT_QUAL + 33]) * l_seq
        else:
            qual = bytes((q + 33) & 0xFF for q in qual)
        if flag & 0x10:
            seq = seq.translate(_SEQ_COMP)[::-1]
            qual = qual[::-1]
        yield b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def write_fastq(path, out_path, batch=1 << 12):
    """fastq_records(path) -> the file out_path."""
    with open(out_path, "wb") as out:
        buf = []
        for rec in fastq_records(path):
            buf.append(rec)
            if len(buf) >= batch:
                out.write(b"".join(buf))
                buf = []
        out.write(b"".join(buf))


def warn_about(path, collating=False):
    """The warnings a BAM input gets on stderr: a coordinate-sorted file (a read's alignments are not adjacent, so the result is
    that of its SAM text, which breaks the same assumption) unless its records are being collated by read (`--collate`), and a
    missing BGZF end-of-file block (accepted, as samtools does)."""
    rd = BamReader(path)
    rd.fh.close()
    for ln in rd.text.splitlines():
        if not collating and ln.startswith("@HD") and "SO:coordinate" in ln.split("\t"):
            print("Warning: %s is sorted by coordinate; a read's alignments are expected next to each other (sort by name)"
                  ", or pass --collate auto to regroup them by read" % path, file=sys.stderr)
            break
    if _is_gzip(path) and not has_eof_block(path):
        print("Warning: %s has no BGZF end-of-file block (a truncated file?)" % path, file=sys.stderr)
