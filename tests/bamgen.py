"""Test helper: SAM lines -> BAM bytes (SAM specification §4.2), pure Python (struct + zlib).

The reference list is the header's @SQ names, then every other RNAME / RNEXT the records use, in order of first use.  Integer
tags are stored in the smallest type that holds them, as samtools does (c C s S i I); A, f, Z, H and B tags as written.  The
BGZF members hold at most `block` bytes of the stream each (so records straddle members), with the BC extra field and the
end-of-file block unless eof=False."""
import re
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
_INT_TYPES = (("c", "<b", -128, 127), ("C", "<B", 0, 255), ("s", "<h", -32768, 32767), ("S", "<H", 0, 65535),
              ("i", "<i", -2 ** 31, 2 ** 31 - 1), ("I", "<I", 0, 2 ** 32 - 1))
_HEADER = re.compile(r"@[A-Z][A-Z](\t|$)")
_B_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def _lines(sam):
    if isinstance(sam, (bytes, str)):
        sam = sam.decode("latin-1") if isinstance(sam, bytes) else sam
        return [ln for ln in sam.split("\n") if ln]
    return [ln.rstrip("\n") for ln in sam if ln.rstrip("\n")]


def _tag(t):
    tag, ty, val = t[:2].encode("latin-1"), t[3], t[5:]
    if ty == "i":
        v = int(val)
        for code, fmt, lo, hi in _INT_TYPES:
            if lo <= v <= hi:
                return tag + code.encode() + struct.pack(fmt, v)
        raise ValueError("integer tag out of range: %s" % t)
    if ty == "A":
        return tag + b"A" + val.encode("latin-1")[:1]
    if ty == "f":
        return tag + b"f" + struct.pack("<f", float(val))
    if ty in "ZH":
        return tag + ty.encode() + val.encode("latin-1") + b"\0"
    if ty == "B":
        sub, *vals = val.split(",")
        conv = float if sub == "f" else int
        return tag + b"B" + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(_B_FMT[sub], conv(v)) for v in vals)
    raise ValueError("tag type %r" % ty)


def record(f, refid, mate_refid):
    """The fields of one SAM line (a list of str) -> one BAM record, block_size first."""
    qname, flag, pos, mapq, cigar = f[0], int(f[1]), int(f[3]), int(f[4]), f[5]
    ops = []
    if cigar != "*":
        num = ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                ops.append((int(num) << 4) | CIGAR_OPS.index(ch))
                num = ""
    seq = "" if f[9] == "*" else f[9]
    packed = bytearray((len(seq) + 1) // 2)
    for k, ch in enumerate(seq):
        packed[k >> 1] |= SEQ_CODES.get(ch.upper(), 15) << (4 * (1 - (k & 1)))
    qual = b"\xff" * len(seq) if f[10] == "*" else bytes((ord(c) - 33) & 0xFF for c in f[10])
    name = qname.encode("latin-1") + b"\0"
    body = struct.pack("<iiBBHHHIiii", refid, pos - 1, len(name), mapq, 4680, len(ops), flag, len(seq), mate_refid, int(f[7]) - 1,
                       int(f[8]))
    body += name + b"".join(struct.pack("<I", o) for o in ops) + bytes(packed) + qual + b"".join(_tag(t) for t in f[11:])
    return struct.pack("<I", len(body)) + body


def encode(sam):
    """SAM text or lines -> (the uncompressed BAM stream, the header's byte count, the reference names)."""
    lines = _lines(sam)
    header = [ln for ln in lines if _HEADER.match(ln)]
    body = [ln.split("\t") for ln in lines if not _HEADER.match(ln)]  # (a record may have a QNAME that starts with '@')
    names, index = [], {}

    def ref(name):
        if name not in index:
            index[name] = len(names)
            names.append(name)
        return index[name]

    for ln in header:
        if ln.startswith("@SQ"):
            for fld in ln.split("\t"):
                if fld.startswith("SN:"):
                    ref(fld[3:])
    for f in body:
        if f[2] != "*":
            ref(f[2])
        if f[6] not in ("*", "="):
            ref(f[6])
    text = "".join(ln + "\n" for ln in header).encode("latin-1")
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(names))]
    for nm in names:
        nb = nm.encode("latin-1") + b"\0"
        out += [struct.pack("<i", len(nb)), nb, struct.pack("<i", 50000)]
    hdr = b"".join(out)
    recs = []
    for f in body:
        rid = -1 if f[2] == "*" else index[f[2]]
        mid = -1 if f[6] == "*" else (rid if f[6] == "=" else index[f[6]])
        recs.append(record(f, rid, mid))
    return hdr + b"".join(recs), len(hdr), names


def bgzf(data, block=65280, eof=True, level=6):
    """Bytes -> BGZF members of at most `block` input bytes each (+ the end-of-file block)."""
    out = []
    for i in range(0, len(data), block):
        chunk = data[i:i + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        bsize = 18 + len(comp) + 8
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + comp
                   + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def sam_to_bam(sam, block=65280, eof=True, level=6):
    return bgzf(encode(sam)[0], block=block, eof=eof, level=level)


def bgzf_text(text, block=65280):
    """A SAM text as BGZF (what `bgzip` writes), for comparisons with the BAM of the same lines."""
    return bgzf(text.encode("latin-1") if isinstance(text, str) else text, block=block)
