"""SAM / PAF text whose BYTES lie where the tokeniser's fast paths change (mg_ingest.hip), and what the definition makes of it.
Shared by test_sam_cases_host.py (every family reaches what it claims) and test_gpu_sam_geometry.py (the kernels).

expected() is the definition over a text: map_and_profile._Tokeniser (PAF: _tokenise_paf_from) for the records and the names,
coverage.placement, identity.edit_of and variants.entries_and_pool for the side arrays.  All it adds is the splitting rule: lines
end at b"\\n" and nowhere else, and a trailing unterminated line is a line.

A family is a function that returns [(name, text bytes)].  Three inputs on which the device is knowingly the stricter parser are
kept out of every family BY CONSTRUCTION ("Known departures of the text tokeniser"; DEPARTURES holds one line of
each, and test_sam_cases_host.py shows what the definition does with it):

  * '_' inside a FLAG or NM number (int() takes it);
  * non-ASCII white space (U+0085, U+00A0, ...) as a separator (str.split() takes it);
  * non-ASCII letters or digits inside a CIGAR (str.isalpha() / int() take them).

For the same reason SEQ is ASCII (len(SEQ) counts characters, the device bytes) and PAF's number columns hold [+-]digits only.
"""
import re
from collections import namedtuple

import numpy as np

from metalign_amd import _hip
from metalign_amd import coverage as cv
from metalign_amd import identity as idn
from metalign_amd import map_and_profile as mp
from metalign_amd import variants as var

# accession names of 1 to 17 bytes (RNAME is a field like any other), one inside another, and one with a blank (PAF only)
ACCS = [("X%dabcdefghijklmnop" % k)[:k] for k in range(1, 18)] + ["sp ace"]
IDX = {"Unmapped": 0}
IDX.update({a: i + 1 for i, a in enumerate(ACCS)})
NAMES = ["Unmapped"] + ACCS  # row order, for Hip.acc_index

SEPS = " \t\x0b\x0c\r\x1c\x1d\x1e\x1f"                      # str.split()'s ASCII white space without '\n'
LOW = bytes(range(0x01, 0x09)) + bytes(range(0x0e, 0x1c))    # below 0x21 and NOT white space
E_ACUTE = "\u00e9".encode("utf-8")                           # two bytes, both >= 0x80
MAX_SEQLEN = _hip.MAX_SEQLEN

Expected = namedtuple("Expected", "recs names last_qname qnames places edits bases error")
# error: None, or (exception type, message, 0-based line); then every other field is None
KIND_OF = {KeyError: 1, IndexError: 2, ValueError: 3, ZeroDivisionError: 4, OverflowError: 5}  # include/metalign_hip.h

DEPARTURES = [
    ("underscore in FLAG", b"q\t1_6\tX\t1\t0\t5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\n"),
    ("underscore in NM", b"q\t0\tX\t1\t0\t5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:1_0\n"),
    ("U+0085 as a separator", "q\u00850\tX\t1\t0\t5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\n".encode("utf-8")),
    ("U+00A0 as a separator", "q\t0\tX\t1\t0\t5M\t*\t0\t0\tACGTA\u00a0IIIII\tNM:i:0\n".encode("utf-8")),
    ("non-ASCII letter in CIGAR", "q\t0\tX\t1\t0\t5\u00e9\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\n".encode("utf-8")),
    ("non-ASCII digit in CIGAR", "q\t0\tX\t1\t0\t\u0665M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0\n".encode("utf-8")),
]


def ascii_fields(line_bytes):
    """The fields the device sees: maximal runs of bytes outside str.split()'s ASCII white space."""
    white = (SEPS + "\n").encode()
    return [f for f in re.split(b"[" + re.escape(white) + b"]+", bytes(line_bytes)) if f]


def split_lines(text_bytes):
    """The lines of a text, decoded: cut at b"\\n" only; what follows the last newline is a line unless it is empty."""
    parts = bytes(text_bytes).split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return [p.decode("utf-8") for p in parts]


def expected(text_bytes, idx, prev_qname="", paf=False):
    lines = split_lines(text_bytes)
    names, qnames = [], []
    try:
        at = 0
        if paf:
            parts, prev = [], prev_qname
            for at, ln in enumerate(lines):
                got, prev = mp._tokenise_paf_from([ln], idx, prev, names=names)
                parts.append(got)
                if len(got):
                    qnames.append(ln.rstrip("\r\n").split("\t")[0])
            recs = np.concatenate(parts) if parts else np.zeros(0, dtype=_hip.REC_DTYPE)
        else:
            tk = mp._Tokeniser(idx)
            tk.prev = prev_qname
            for at, ln in enumerate(lines):
                tk.feed(ln)
            recs, prev, names = tk.records(), tk.prev, tk.names
    except (KeyError, IndexError, ValueError, ZeroDivisionError, OverflowError) as e:
        return Expected(None, None, None, None, None, None, None, (type(e), str(e), at))
    if paf:
        return Expected(recs, mp._pack_names(names), prev, qnames, None, None, None, None)
    fields = [f for f in map(cv.retained_fields, lines) if f is not None]
    assert len(fields) == len(recs)
    places = np.array([cv.placement(f) for f in fields], dtype=_hip.PLACE_DTYPE) if fields else np.zeros(0, dtype=_hip.PLACE_DTYPE)
    edits = np.array([idn.edit_of(f) for f in fields], dtype=_hip.EDIT_DTYPE) if fields else np.zeros(0, dtype=_hip.EDIT_DTYPE)
    ent, pool = var.entries_and_pool(fields)
    ent = np.array(ent, dtype=_hip.BASES_DTYPE) if ent else np.zeros(0, dtype=_hip.BASES_DTYPE)
    return Expected(recs, mp._pack_names(names), prev, [f[0] for f in fields], places, edits, (ent, pool), None)


# ------------------------------------------------------------------------------------------------------------------------------
# lines
# ------------------------------------------------------------------------------------------------------------------------------
def _b(x):
    return x if isinstance(x, bytes) else str(x).encode("utf-8")


def sam_line(q, flag=0, rname="X", pos=1, mapq=60, cigar="5M", rnext="*", pnext=0, tlen=0, seq="ACGTA", qual="IIIII",
             tags=("NM:i:1",), sep=b"\t", nfields=None):
    """A SAM line without its newline; nfields: only its first so many fields."""
    f = [_b(x) for x in (q, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual)] + [_b(t) for t in tags]
    return sep.join(f if nfields is None else f[:nfields])


def paf_line(q, qlen=10, qs=0, qe=10, strand="+", tname="X", tlen=100, ts=0, te=10, nmatch=9, alen=10, mapq=60, tags=(),
             nfields=None):
    f = [_b(x) for x in (q, qlen, qs, qe, strand, tname, tlen, ts, te, nmatch, alen, mapq)] + [_b(t) for t in tags]
    return b"\t".join(f if nfields is None else f[:nfields])


# ------------------------------------------------------------------------------------------------------------------------------
# window_edges: where the '\n' bytes lie (k_count_newlines, k_mark_newlines)
# ------------------------------------------------------------------------------------------------------------------------------
class _Text:
    """A text of retained lines with names of their own ('R'), lines that raise KeyError ('E') and junk, in SAM or PAF."""

    def __init__(self, paf):
        self.paf, self.buf, self.n = paf, bytearray(), 0

    def line(self, kind="R"):
        self.n += 1
        q, acc = "%c%d" % ("qrstuvw"[self.n % 7], self.n), ("NOPE" if kind == "E" else ACCS[self.n % 9])
        if self.paf:
            return paf_line(q, tname=acc, nmatch=self.n % 10)
        return sam_line(q, 16 * (self.n % 2), acc, 1 + self.n, 0, "%dM" % (1 + self.n % 9), "*", 0, 0, "A", "I", ("NM:i:%d" % (self.n % 4),), b" ")

    def add(self, kind="R", nl=b"\n"):
        self.buf += self.line(kind) + nl
        return self

    def raw(self, data):
        self.buf += data
        return self

    def land(self, target, kind="R"):
        """The next line's '\\n' at byte `target`: junk (a line of one field) in front of it takes up the room."""
        ln = self.line(kind)
        gap = target - len(self.buf) - len(ln)
        assert gap >= 0, (target, len(self.buf))
        if gap:
            self.buf += b"j" * (gap - 1) + b"\n"
        self.buf += ln + b"\n"
        assert self.buf[target] == 0x0A
        return self

    def fill(self, upto, nl=b"\n"):
        while len(self.buf) < upto:
            self.add("R", nl)
        return self

    def bytes(self):
        return bytes(self.buf)


def window_edges(paf=False):
    def T():
        return _Text(paf)
    one = len(T().line())  # 29 bytes of SAM, 23 of PAF: a retained line of one-byte fields
    out = [("empty", b""), ("one byte, no newline", b"x"), ("retained line, no newline", T().add(nl=b"").bytes()),
           ("retained line", T().add().bytes()), ("CRLF", T().add(nl=b"\r\n").bytes()),
           ("CRLF around", T().raw(b"\r\n\r\n").add(nl=b"\r\n").raw(b"\r\n").bytes())]
    for k in (1, 2, 15, 16, 17, 31, 32, 33, 48):
        out.append(("%d newlines and nothing else" % k, b"\n" * k))
    for k in range(0, 48 - one):  # the line, and so its newline, at every offset a text of 48 bytes has room for
        out.append(("%d newlines, a retained line" % k, T().raw(b"\n" * k).add().bytes()))
        if k + len(T().line("E")) < 48:
            out.append(("%d newlines, a line that raises" % k, T().raw(b"\n" * k).add("E").bytes()))  # (the error's line number counts them)
        out.append(("%d newlines, a retained line, no final newline" % k, T().raw(b"\n" * k).add(nl=b"").bytes()))
        out.append(("a retained line up to byte 48, %d newlines" % k, T().add().raw(b"\n" * (48 - one - 1 - k)).bytes()))
    # more than two index blocks of 4096 bytes (256 windows): newlines of retained lines on the last lane's last byte (1023), on a
    # block's last byte (4095, 8191) and the next one's first (4096, 8192); a window of nothing but newlines
    a = T().fill(600).land(1023).add().fill(3800).land(4095).add().fill(6000).raw(b"\n" * 40).add().fill(7900).land(8191).fill(9100)
    out.append(("block ends", a.bytes()))
    b = T().fill(700).land(1024).fill(3900).land(4096).fill(5000).raw(b"\n" * 16).fill(8000).land(8192).fill(9000).add(nl=b"")
    out.append(("block starts, no final newline", b.bytes()))
    c = T().fill(1000, b"\r\n").raw(b"\n" * 33).fill(4000).land(4095).raw(b"\n").fill(8100, b"\r\n").land(8191).raw(b"\n\n").fill(9000).add("E").add()
    out.append(("CRLF, runs, a line that raises behind two blocks", c.bytes()))
    d = T().raw(b"\n" * 4095).add().raw(b"\n" * 4200).add("E")
    out.append(("blocks of newlines, a line that raises", d.bytes()))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# field_alignment: where fields start and end (scan_to_ws: head, 8-byte body with borrow candidates, tail)
# ------------------------------------------------------------------------------------------------------------------------------
def _len_for(d, lo, hi, bump):
    """A length congruent to d modulo 8 within [lo, hi]; bump: the next one up where there is one."""
    n = lo + (d - lo) % 8
    if bump and n + 8 <= hi:
        n += 8
    if bump > 1 and n + 8 <= hi:
        n += 8
    return n


def _odd_bytes(n, salt):
    """n bytes that are not white space: printable ones, bytes below 0x21, '!' behind one (a borrow candidate) and two-byte letters."""
    out = bytearray()
    k = salt
    while len(out) < n:
        room = n - len(out)
        pick = k % 4
        if pick == 0 and room >= 2:
            out += E_ACUTE
        elif pick == 1:
            out.append(LOW[k % len(LOW)])
            if room >= 2:
                out += b"!"
        else:
            out.append(0x30 + (k * 7) % 75)  # '0' .. 'z'
        k += 1
    if out[0] == 0x40:
        out[0] = 0x41  # (a line that starts with '@' is a header line)
    return bytes(out)


def _cigar_for(nseq, n, salt):
    """A CIGAR of exactly n bytes (n >= 2) whose M, I, S and X lengths sum to nseq where that fits, padded with leading zeros."""
    rich = None
    if nseq >= 6:
        a = 1 + salt % (nseq - 4)
        rest = nseq - a - 1 - 1
        b = 1 + salt % rest if rest > 1 else rest
        rich = "%dM1I%d%s2%s%dS" % (a, b, "MX"[salt % 2], "DN"[salt % 2], nseq - a - 1 - b) if nseq - a - 1 - b > 0 else None
    for c in (rich, "%dM" % nseq, "9M"):
        if c is not None and len(c) <= n:
            return "0" * (n - len(c)) + c
    raise AssertionError((nseq, n))


def field_alignment():
    """Line (s, d): QNAME starts at residue s modulo 8 (leading white space makes up for where the line begins), every field's length
    is d modulo 8, the separators depend on (d, field) only: so every field starts and ends on every residue."""
    buf = bytearray()
    n = 0
    for d in range(8):
        for s in range(8):
            n += 1
            bump = (s + d) % 3
            lens = [_len_for(d, 1, 17, bump), _len_for(d, 1, 17, bump), _len_for(d, 1, 17, (s + 1) % 3), _len_for(d, 1, 17, s % 2),
                    _len_for(d, 1, 17, bump), _len_for(d, 2, 17, (s + 2) % 3), _len_for(d, 1, 17, bump), _len_for(d, 1, 17, s % 2),
                    _len_for(d, 1, 17, bump), _len_for(d, 1, 17, (s + d + 1) % 3), _len_for(d, 1, 17, bump), _len_for(d, 6, 17, s % 2)]
            flags = [f for f in (0, 16, 256, 99, 2048, 147, 272, 1, 3, 83) if len(str(f)) <= lens[1]]
            flag = flags[(s + d) % len(flags)]
            twelfth = ("NM:i:", "AS:i:", "NM:i:+", "XS:i:-")[(s + 2 * d) % 4][:max(5, min(6, lens[11] - 1))]
            twelfth += str((n * 3) % 10).rjust(lens[11] - len(twelfth), "0")
            fields = [_odd_bytes(lens[0], n), _b(str(flag).rjust(lens[1], "0")), _b(ACCS[lens[2] - 1]),
                      _b(str(max(1, (1 + n * 37) % 10 ** min(lens[3], 4))).rjust(lens[3], "0")), _b("6" * lens[4]), _b(_cigar_for(lens[9], lens[5], n)),
                      _b("=" * lens[6]), _b("7" * lens[7]), _b("-" + "8" * (lens[8] - 1) if lens[8] > 1 else "0"),
                      _b("".join("ACGTNacgtRY"[(n + j * (1 + n % 5)) % 11] for j in range(lens[9]))), _odd_bytes(lens[10], n + 5),
                      _b(twelfth)]
            # tags behind the twelfth field: values with odd bytes, and the NM:i: k_sam_edit looks for behind them
            tags = [b"XA:Z:" + _odd_bytes(3 + (n * 5) % 14, n + 1), b"ZZ:Z:" + bytes([LOW[n % len(LOW)]])][: n % 3]
            if not twelfth.startswith("NM:i:"):
                tags.append(b"NM:i:%d" % (n % 7))
            line = bytearray()
            lead = (s - len(buf)) % 8
            for j in range(lead):
                line.append(ord(SEPS[(n + j) % len(SEPS)]))
            for i, f in enumerate(fields + tags):
                if i:
                    run = 1 + ((i + d) % 3 if (i * 3 + d) % 4 == 0 else 0)
                    for j in range(run):
                        line.append(ord(SEPS[(i + d + j * 4) % len(SEPS)]))
                line += f
            for j in range(n % 4):
                line.append(ord(SEPS[(n + 2 * j) % len(SEPS)]))  # trailing white space
            buf += line + b"\n"
    text = bytes(buf)
    # a byte below 0x21 that is no white space directly before and directly after a real separator (one 8-byte word holds all three)
    edge = sam_line(b"rd\x01", 0, "X2", 7, 60, "5M", "*", 0, 0, b"ACGTA", b"\x02III\x03", (b"NM:i:2", b"\x05X:Z:\x06", b"XB:Z:a\x1b")) + b"\n"
    return [("every residue", text), ("low bytes around a separator", edge * 3)]


def field_spans(text):
    """{(field 1 .. 12, start modulo 8, end modulo 8)} over the retained lines of a text whose separators are ASCII."""
    got, at = set(), 0
    white = set(SEPS.encode())
    for raw in bytes(text).split(b"\n"):
        p, k = 0, 0
        while k < 12:
            while p < len(raw) and raw[p] in white:
                p += 1
            if p >= len(raw):
                break
            b = p
            while p < len(raw) and raw[p] not in white:
                p += 1
            k += 1
            got.add((k, (at + b) % 8, (at + p) % 8))
        at += len(raw) + 1
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# field_counts: how many fields, which error, which numbers (k_sam_parse's decisions)
# ------------------------------------------------------------------------------------------------------------------------------
ERROR_ORDER = ["flag", "key", "cigar", "index", "nm", "zero", "overflow"]
ERROR_TYPE = {"flag": ValueError, "key": KeyError, "cigar": ValueError, "index": IndexError, "nm": ValueError,
              "zero": ZeroDivisionError, "overflow": OverflowError}


def error_line(q, kinds):
    """A line that has every defect in `kinds` at once; the definition raises for the first of them in ERROR_ORDER."""
    kinds = set(kinds)
    assert not {"index", "nm"} <= kinds and not {"zero", "overflow"} <= kinds
    cigar = {(False, False, False): "5M", (True, False, False): "3M2=", (False, True, False): "40", (False, False, True): "4294967296M",
             (True, True, False): "5=", (True, False, True): "4294967296M3="}[("cigar" in kinds, "zero" in kinds, "overflow" in kinds)]
    return sam_line(q, "zz" if "flag" in kinds else 0, "NOPE.1" if "key" in kinds else "X3a", 9, 60, cigar,
                    tags=("NM:i:" if "nm" in kinds else "NM:i:3", "XS:i:1"), nfields=11 if "index" in kinds else None)


def error_sets():
    one = [(k,) for k in ERROR_ORDER]
    two = [(a, b) for i, a in enumerate(ERROR_ORDER) for b in ERROR_ORDER[i + 1:] if (a, b) not in (("index", "nm"), ("zero", "overflow"))]
    return one + two


def field_counts():
    ok = sam_line("ok1") + b"\n"
    good = bytearray()
    for nf in range(0, 14):
        for form, (flag, cigar) in (("retained", (0, "5M")), ("star", (16, "*")), ("unmapped", (4 + 16 * (nf % 2), "5M"))):
            if form == "retained" and 6 <= nf <= 11:
                continue  # (IndexError: texts of their own below)
            good += sam_line("n%d%s" % (nf, form[0]), flag, "X2", 5, 60, cigar, tags=("NM:i:1", "XS:i:2"), nfields=nf) + b"\n"
    good += b"@HD\tVN:1.6\n" + b"@" + sam_line("x") + b"\n" + b" @" + sam_line("x", sep=b" ") + b"\n" + b"@\n"
    out = [("0 to 13 fields that raise nothing, header lines", bytes(good))]
    for nf in range(6, 12):
        out.append(("retained line of %d fields" % nf, ok * 3 + sam_line("short", nfields=nf) + b"\n" + ok))
    for kinds in error_sets():
        out.append(("raises: " + " and ".join(kinds), ok * 2 + error_line("bad", kinds) + b"\n" + ok))
    out.append(("bad FLAG on a line with * CIGAR", ok + sam_line("bad", "1x", cigar="*") + b"\n"))
    # two bad lines, in blocks of their own (256 lines a block): the lower line number wins
    for first, second in (("key", "cigar"), ("zero", "key")):
        lines = [b"x"] * 700
        lines[3], lines[300], lines[650] = ok.rstrip(b"\n"), error_line("b1", (first,)), error_line("b2", (second,))
        out.append(("%s at line 300, %s at line 650" % (first, second), b"\n".join(lines) + b"\n"))
        lines[300], lines[650] = lines[650], lines[300]
        out.append(("%s at line 300, %s at line 650" % (second, first), b"\n".join(lines) + b"\n"))
    big = next(v for v in range(999999999999999, 0, -1) if not v & 4 and v & 0xFF0)
    flags = b"".join(sam_line("f%d" % i, f) + b"\n" for i, f in enumerate(("+16", "-1", "-8", "4095", "4096", "0016", str(big), "-" + str(big))))
    out.append(("FLAG forms", flags))
    out.append(("NM forms that parse", b"".join(sam_line("m%d" % i, tags=(t, "NM:i:9")) + b"\n" for i, t in enumerate(("NM:i:+3", "NM:i:-0", "NM:i:-7", "NM:i:007", "XX:i:12")))))
    for t in ("NM:i:", "XX:Z:NM:i:7", "NM:i", "NM:i:+", "NM:i:3x"):
        out.append(("twelfth field " + t, ok + sam_line("bad", tags=(t,)) + b"\n" + ok))
    letters = "".join("%d%c" % (1 + i % 3, 65 + i) for i in range(26))
    cigars = [letters, letters.lower(), "M5M", "5MD", "5M3", "3m2d4M", "4294967295M", "4294967290M5S", "2147483648M2147483647D", "00000000000000000005M"]
    out.append(("CIGAR forms", b"".join(sam_line("c%d" % i, cigar=c) + b"\n" for i, c in enumerate(cigars))))
    for c in ("0M", "4294967296M", "4294967295M1S", "12", "5M=", "*M"):
        out.append(("CIGAR " + c, ok + sam_line("bad", cigar=c) + b"\n" + ok))
    out.append(("SEQ * and of one base", sam_line("s0", seq="*", qual="*") + b"\n" + sam_line("s1", cigar="1M", seq="G", qual="I") + b"\n"))
    out.append(("SEQ of the longest length", ok + sam_line("long", cigar="%dM" % MAX_SEQLEN, seq=b"ACGTTGCA" * (MAX_SEQLEN // 8) + b"ACGTTGC", qual="*") + b"\n" + ok))
    out.append(("SEQ one longer than that", ok + sam_line("long", cigar="%dM" % (MAX_SEQLEN + 1), seq=b"ACGTTGCA" * ((MAX_SEQLEN + 1) // 8), qual="*") + b"\n" + ok))
    return out


def field_count_of(line):
    return len(line.strip().split())


# ------------------------------------------------------------------------------------------------------------------------------
# qnames: k_sam_emit's comparison, k_name_gather's groups of 16 lanes, the QNAME carried in and out
# ------------------------------------------------------------------------------------------------------------------------------
QNAME_LENGTHS = [1, 15, 16, 17, 254, 255, 300]
_ALNUM = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"


def base_name(n):
    return "".join(_ALNUM[(i * 7 + n) % 62] for i in range(n))


def qnames():
    out = []
    for n in QNAME_LENGTHS:
        q = base_name(n)
        first = ("#" if q[0] != "#" else "$") + q[1:]
        last = q[:-1] + ("#" if q[-1] != "#" else "$")
        seq = [q, q, None, q, first, q, last]            # equal, equal across other lines, first byte, last byte
        seq += [q[:-1], q] if n > 1 else []               # a proper prefix behind the longer name, the longer name behind it
        seq += [q + "x", q, q + "x", q + "x"]             # one byte longer, and back
        lines = []
        for i, name in enumerate(seq):
            if name is None:  # lines that are not retained, with names of their own
                lines += [sam_line("other", 4), sam_line(q + "y", 0, cigar="*"), b"short line", b"@CO\t" + _b(q)]
            else:
                lines.append(sam_line(name, 16 * (i % 2), ACCS[i % 17], 1 + i, cigar="%dM" % (1 + i), seq="ACGTACGTACGTA"[:1 + i], qual="*",
                                      tags=("NM:i:%d" % (i % 3),)))
        out.append(("names of %d bytes" % n, b"\n".join(lines) + b"\n"))
    return out


def prev_qnames(text):
    """What a qnames text is tokenised after: nothing, its first retained name, that name one byte shorter, one longer, 300 bytes."""
    q = text.split(b"\t", 1)[0].decode()
    return ["", q, q[:-1], q + "x", base_name(300) if q != base_name(300) else base_name(300)[::-1]]


def relations(names):
    """{(relation, length)} over consecutive names; a prefix pair counts for both lengths."""
    got = set()
    for a, b in zip(names, names[1:]):
        if a == b:
            got.add(("equal", len(a)))
        elif len(a) == len(b):
            if a[1:] == b[1:]:
                got.add(("first byte", len(a)))
            if a[:-1] == b[:-1]:
                got.add(("last byte", len(a)))
        elif b.startswith(a):
            got.update({("prefix first", len(a)), ("prefix first", len(b))})
        elif a.startswith(b):
            got.update({("prefix second", len(a)), ("prefix second", len(b))})
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# many_lines: more lines than one pass of the parser's grid (256 threads x 16 blocks per compute unit)
# ------------------------------------------------------------------------------------------------------------------------------
def grid_lines(ncu):
    return 256 * 16 * ncu


def many_lines(ncu, every=4093):
    """-> (text, the indices of its retained lines).  Equal QNAMEs on both sides of the grid's edge, and across line 2 * every."""
    grid = grid_lines(ncu)
    n = grid + 100000
    lines = [b"", b"x"] * (n // 2) + [b""] * (n % 2)
    where = sorted(set(range(0, n, every)) | {n - 1, grid - 2, grid - 1, grid, grid + 1})
    for k, i in enumerate(where):
        name = "edge" if i in (grid - 1, grid) else "r%d" % (k // 2)  # (names come in pairs)
        lines[i] = sam_line(name, 16 * (k % 2), ACCS[k % 17], 1 + k, cigar="%dM" % (1 + k % 9), seq="A", qual="*", tags=("NM:i:0",))
    return b"\n".join(lines) + b"\n", where


# ------------------------------------------------------------------------------------------------------------------------------
# paf_fields: k_paf_parse's decisions
# ------------------------------------------------------------------------------------------------------------------------------
def paf_fields():
    ok = paf_line("ok1") + b"\n"
    good = [paf_line("f11", nfields=11), paf_line("f12"), paf_line("f13", tags=("tp:A:P",)), paf_line("", tags=("cg:Z:10M",)),
            paf_line("", strand="", nmatch="", tags=("cg:Z:8M2I",)), paf_line("read 1", tname="sp ace", mapq="6 0"),
            paf_line("minus", strand="-", tags=("tp:A:S",)), paf_line("twice", tags=("tp:A:S", "tp:A:P")),
            paf_line("twice", tags=("tp:A:P", "xx:i:3", "tp:A:S")), paf_line("five", tags=("tp:A:S", "tp:A:")),
            paf_line("five", tags=("cg:Z:", "cg:Z:9M", "cg:Z")), paf_line("ss", tags=("tp:A:SS",)), paf_line("ss", tags=("tp:AxS",)),
            paf_line("cg", qlen=30, qs=2, qe=27, tags=("cg:Z:5M2I3D7N4X1=4", "NM:i:3")), paf_line("cg", tags=("cg:Z:3M", "cg:Z:6M4D")),
            paf_line("back", qlen=20, qs=15, qe=5, tags=("cg:Z:10M",)), paf_line("neg", qlen=20, qs=-3, qe=7, tags=("cg:Z:10M",)),
            paf_line("plus", qlen="+12", qs="+0", qe="-0", nmatch="+7"), paf_line("tabs", tags=("", "", "tp:A:S", "")),
            paf_line("lower", tags=("cg:Z:4m6M",)), b"", b"\t" * 10]
    out = [("lines that raise nothing", b"\n".join(good) + b"\n"), ("CRLF", b"\r\n".join(good[:8]) + b"\r\n"),
           ("no final newline", ok + paf_line("last", tags=("tp:A:S",)))]
    bad = [("zero total", paf_line("bad", qlen=0)), ("zero total from cg", paf_line("bad", qlen=10, qs=0, qe=10, tags=("cg:Z:5",))),
           ("unknown target", paf_line("bad", tname="NOPE")), ("empty target", paf_line("bad", tname="")),
           ("empty matches without cg", paf_line("bad", nmatch="")), ("a number that is none", paf_line("bad", qs="1x")),
           ("negative length", paf_line("bad", qlen=-10)), ("negative matches", paf_line("bad", nmatch=-4)),
           ("zero total and unknown target", paf_line("bad", qlen=0, tname="NOPE")),
           ("no number and zero total", paf_line("bad", qlen=0, qe="")), ("twelve empty fields", b"\t" * 11)]
    for name, ln in bad:
        out.append(("raises: " + name, ok * 2 + ln + b"\n" + ok))
    return out
