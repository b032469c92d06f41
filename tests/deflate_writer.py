"""A DEFLATE (RFC 1951) / gzip (RFC 1952) / BGZF *assembler*: test infrastructure, no compression logic.  The caller says what goes on
the wire — block types, code lengths, how the length lists are run-length coded, which symbol and extra bits stand for a length, the
padding bits of a stored block — and gets the bytes; `expand` says what the same tokens MEAN without a single bit-level operation.
zlib's INFLATER reads all of RFC 1951, its deflater writes a narrow corner of it: with this module the inflaters of the library are held
to zlib on streams as libdeflate, igzip and pigz write them, and on streams nobody writes.  `corpus()` is that set of streams.

Tokens (of `Stream.fixed` / `Stream.dynamic` and `expand`):
    int 0..255                       a literal
    bytes                            a run of literals
    (length, distance)               a match; (258, distance, True): length 258 as symbol 284 with extra bits 31
    ("sym", ls, lx, ds, dx)          literal/length symbol ls with extra bits lx, then (ds is not None) distance symbol ds with extra bits dx —
                                     any symbol the code has, 286 / 287 / 30 / 31 included
    ("bits", value, n)               n raw bits
    EOB                              end of block (blocks end with one unless eob=False)
"""
import bisect
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

EOB = ("eob",)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# the decoder's batch: output bytes and queued symbols (mg_inflate_core.h; tests/test_inflate_foreign_host.py holds the two files together)
kBatchBytes, kBatchSyms = 4096, 256


def length_symbol(length, alt258=False):
    """-> (symbol, extra bits' value) of a match length"""
    assert 3 <= length <= 258
    if length == 258:
        return (284, 31) if alt258 else (285, 0)
    s = bisect.bisect_right(LEN_BASE, length) - 1
    return 257 + s, length - LEN_BASE[s]


def distance_symbol(dist):
    assert 1 <= dist <= 32768
    s = bisect.bisect_right(DIST_BASE, dist) - 1
    return s, dist - DIST_BASE[s]


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lens):
    """Code lengths -> the codes as their bits go on the wire (LSB first), RFC 1951 3.2.2.  Lengths that are no prefix code (over-subscribed)
    still get codes — of a header that is meant to be refused."""
    return list(_canonical(tuple(lens)))


@functools.lru_cache(maxsize=256)
def _canonical(lens):
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        out.append(_rev(nxt[l] & ((1 << l) - 1), l))
        nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 = a complete code"""
    return sum(32768 >> l for l in lens if l)


class BitWriter:
    """LSB-first bits."""

    def __init__(self):
        self.parts = []          # ("bits", values u64[], counts u8[]) | ("bytes", bytes)
        self._v, self._n = [], []
        self.nbits = 0

    def bits(self, value, n):
        assert 0 <= n <= 57 and 0 <= value < (1 << n)
        if n:
            self._v.append(value)
            self._n.append(n)
            self.nbits += n

    def _flush(self):
        if self._v:
            self.parts.append(("bits", np.array(self._v, dtype=np.uint64), np.array(self._n, dtype=np.int64)))
            self._v, self._n = [], []

    def bits_array(self, values, counts):
        self._flush()
        counts = np.asarray(counts, dtype=np.int64)
        self.parts.append(("bits", np.asarray(values, dtype=np.uint64), counts))
        self.nbits += int(counts.sum())

    def align(self, pad=0):
        """to the byte boundary; the bits skipped take the low bits of pad"""
        n = -self.nbits % 8
        self.bits(pad & ((1 << n) - 1), n)
        return n

    def raw_bytes(self, data):
        assert self.nbits % 8 == 0
        self._flush()
        self.parts.append(("bytes", bytes(data)))
        self.nbits += 8 * len(data)

    def getvalue(self):
        """the bytes (the last one filled with zero bits)"""
        self._flush()
        out, pending = [], []

        def pack():
            if pending:
                out.append(np.packbits(np.concatenate(pending), bitorder="little").tobytes())
                pending.clear()
        for p in self.parts:
            if p[0] == "bytes":
                pack()  # (raw_bytes asserted the alignment)
                out.append(p[1])
                continue
            _, values, counts = p
            for a in range(0, len(counts), 1 << 18):
                v, c = values[a:a + (1 << 18)], counts[a:a + (1 << 18)]
                ends = np.cumsum(c)
                off = np.arange(int(ends[-1]) if len(ends) else 0, dtype=np.int64) - np.repeat(ends - c, c)
                pending.append(((np.repeat(v, c) >> off.astype(np.uint64)) & np.uint64(1)).astype(np.uint8))
        pack()
        return b"".join(out)


def _encode_tokens(w, tokens, lit_lens, dist_lens, eob=True):
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    lc_a, ll_a = np.array(lc[:256] + [0] * max(0, 256 - len(lc)), dtype=np.uint64), np.array(lit_lens[:256] + [0] * max(0, 256 - len(lit_lens)), dtype=np.int64)

    def lsym(s, xv):
        assert s < len(lit_lens) and lit_lens[s], "literal/length symbol %d has no code" % s
        w.bits(lc[s], lit_lens[s])
        if 257 <= s <= 285:
            w.bits(xv, LEN_EXTRA[s - 257])

    def dsym(s, xv):
        assert s < len(dist_lens) and dist_lens[s], "distance symbol %d has no code" % s
        w.bits(dc[s], dist_lens[s])
        if s < 30:
            w.bits(xv, DIST_EXTRA[s])
    for t in list(tokens) + ([EOB] if eob else []):
        if isinstance(t, int):
            lsym(t, 0)
        elif isinstance(t, (bytes, bytearray)):
            a = np.frombuffer(bytes(t), dtype=np.uint8)
            assert a.size == 0 or ll_a[a].min() > 0, "a literal of the run has no code"
            w.bits_array(lc_a[a], ll_a[a])
        elif t[0] == "eob":
            lsym(256, 0)
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        elif t[0] == "sym":
            lsym(t[1], t[2])
            if t[3] is not None:
                dsym(t[3], t[4])
        else:
            lsym(*length_symbol(t[0], len(t) > 2 and t[2]))
            dsym(*distance_symbol(t[1]))


class TooFar(Exception):
    pass


def expand(tokens, history=b"", tolerant=False):
    """The bytes the tokens mean (RFC 1951 3.2.3), behind `history` (output of the same member that the tokens may copy from).
    A distance behind the start raises TooFar; tolerant: it reads zeros instead (what a decoder WITHOUT the check would make — the
    trailer of a stream that must be refused is written for that text, so that no CRC check rescues such a decoder)."""
    out = bytearray(history)
    h = len(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        if isinstance(t, (bytes, bytearray)):
            out += t
            continue
        if t[0] in ("eob", "bits"):
            continue
        if t[0] == "sym":
            _, ls, lx, ds, dx = t
            if ls < 256:
                out.append(ls)
                continue
            if ls == 256:
                continue
            if not (257 <= ls <= 285 and ds is not None and ds < 30):
                break  # nothing legal follows
            length, dist = LEN_BASE[ls - 257] + lx, DIST_BASE[ds] + dx
        else:
            length, dist = t[0], t[1]
        if dist > len(out):
            if not tolerant:
                raise TooFar("distance %d with %d bytes there" % (dist, len(out)))
            k = dist - len(out)
            out[:0] = bytes(k)
            h += k
        seg = out[len(out) - dist: len(out) - dist + length]
        out += seg if dist >= length else (seg * (length // dist + 1))[:length]  # (a match that overlaps itself repeats its first dist bytes)
    return bytes(out[h:])


# ---- run-length codings of a list of code lengths (the caller's choice; symbols 16 / 17 / 18) -> [(symbol, extra bits' value)] ----
def rle_none(lengths):
    return [(l, 0) for l in lengths]


def rle_greedy(lengths):
    """the longest run every time (about what encoders do)"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        l = lengths[i]
        run = 1
        while i + run < n and lengths[i + run] == l:
            run += 1
        if l == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
        elif i > 0 and lengths[i - 1] == l and run >= 3:
            r = min(run, 6)
            out.append((16, r - 3))
            i += r
        else:
            out.append((l, 0))
            i += 1
    return out


def rle_random(rng, lengths):
    """any valid coding: at every place one of the choices the format allows"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        l = lengths[i]
        run = 1
        while i + run < n and lengths[i + run] == l:
            run += 1
        ways = ["lit"]
        if l == 0 and run >= 3:
            ways.append("17")
        if l == 0 and run >= 11:
            ways.append("18")
        if i > 0 and lengths[i - 1] == l and run >= 3:
            ways.append("16")
        way = ways[int(rng.integers(0, len(ways)))]
        if way == "lit":
            out.append((l, 0))
            i += 1
        elif way == "17":
            r = int(rng.integers(3, min(run, 10) + 1))
            out.append((17, r - 3))
            i += r
        elif way == "18":
            r = int(rng.integers(11, min(run, 138) + 1))
            out.append((18, r - 11))
            i += r
        else:
            r = int(rng.integers(3, min(run, 6) + 1))
            out.append((16, r - 3))
            i += r
    return out


def flat_code(n):
    """n >= 2 symbols -> lengths of a complete code, as even as can be"""
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def random_code(rng, n, maxbits):
    """n >= 2 symbols -> lengths of a random complete code of at most maxbits bits"""
    assert 2 <= n <= 1 << maxbits
    leaves = [1, 1]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < maxbits]
        i = open_[int(rng.integers(0, len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return [leaves[int(i)] for i in rng.permutation(n)]


def spread(n, symbols, lengths):
    """a list of n code lengths: symbols[i] gets lengths[i], the rest 0"""
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


class Stream:
    """One raw deflate stream, block by block."""

    def __init__(self):
        self.w = BitWriter()
        self.tokens = []  # of all blocks, for expand (a stored block's data is a run of literals)

    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, pad_bits=0, nlen=None):
        assert len(data) <= 65535
        self.header(final, 0)
        self.w.align(pad_bits)
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self.w.raw_bytes(data)
        self.tokens.append(bytes(data))
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.header(final, 1)
        _encode_tokens(self.w, tokens, FIXED_LIT, FIXED_DIST, eob)
        self.tokens += list(tokens)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_syms=None, rle=rle_greedy, eob=True):
        """lit_lens / dist_lens: the code lengths of the two codes (shorter lists are filled with zeros up to hlit / hdist).
        hlit / hdist: how many lengths are sent (default: as few as the format allows — up to the last one that is not zero; at least
        257 / 1; more than 286 / 30, up to 288 / 32, writes the field values that inflaters must refuse).  cl_syms: the run-length coding
        of the hlit + hdist lengths, [(symbol, extra)] (default: rle(the list)); it is written as given, right or wrong.  cl_lens: the 19
        lengths of the code-length code by symbol (default: a flat complete code over the symbols cl_syms uses).  hclen: how many of them
        are sent, in the format's order (default: up to the last that is not zero; at least 4)."""
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max([257] + [i + 1 for i, l in enumerate(lit_lens) if l])
        if hdist is None:
            hdist = max([1] + [i + 1 for i, l in enumerate(dist_lens) if l])
        assert 257 <= hlit <= 288 and 1 <= hdist <= 32
        lit_lens = (lit_lens + [0] * hlit)[:hlit]
        dist_lens = (dist_lens + [0] * hdist)[:hdist]
        if cl_syms is None:
            cl_syms = rle(lit_lens + dist_lens)
        if cl_lens is None:
            used = sorted({s for s, _ in cl_syms})
            if len(used) < 2:
                used = sorted(set(used) | {0 if 0 not in used else 1})
            cl_lens = spread(19, used, flat_code(len(used)))
        assert len(cl_lens) == 19 and max(cl_lens) <= 7
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        assert 4 <= hclen <= 19
        self.header(final, 2)
        w = self.w
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cc = canonical(cl_lens)
        for s, x in cl_syms:
            assert cl_lens[s], "code-length symbol %d has no code" % s
            w.bits(cc[s], cl_lens[s])
            w.bits(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        _encode_tokens(w, tokens, lit_lens, dist_lens, eob)
        self.tokens += list(tokens)
        return self

    def block3(self, final=False):
        self.header(final, 3)
        self.w.bits(0x2a5, 10)
        return self

    def raw(self):
        return self.w.getvalue()

    def data(self, history=b"", tolerant=False):
        return expand(self.tokens, history, tolerant)


# ---- wrappers ----
def gzip_member(raw, data, extra=None, name=None, comment=None, hcrc=False):
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def bgzf_block(raw, data):
    assert len(data) <= 65536 and len(raw) + 26 <= 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", zlib.crc32(data), len(data))


BGZF_EOF = bgzf_block(b"\x03\0", b"")


def bgzf(blocks, eof=True):
    """blocks: [(raw stream, its text)], each its own member with a BC field"""
    return b"".join(bgzf_block(r, d) for r, d in blocks) + (BGZF_EOF if eof else b"")


# ---- the two references ----
def zlib_inflate(blob):
    """Every member of a gzip file by zlib's inflater (decompressobj).  zlib.error where zlib refuses the DATA; a stream that only ends early
    is an AssertionError here: no entry of the corpus is meant to be that."""
    out, rest = [], blob
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof, "the stream ends inside a member"
        rest = d.unused_data
    return b"".join(out)


Entry = namedtuple("Entry", "name blob want members bgzf")  # want = None: must be refused


def _check(name, blob, want, members=1, is_bgzf=False):
    """an entry, both references consulted"""
    if want is None:
        try:
            zlib_inflate(blob)
        except zlib.error as e:
            assert "incorrect" not in str(e), "%s: zlib reads the data and refuses only the trailer" % name
            return Entry(name, blob, None, members, is_bgzf)
        raise AssertionError("%s: zlib accepts what the corpus calls illegal" % name)
    got = zlib_inflate(blob)
    assert got == want, "%s: zlib and expand disagree (%d bytes against %d)" % (name, len(got), len(want))
    return Entry(name, blob, want, members, is_bgzf)


# ---- random legal streams ----
def random_tokens(rng, ntok, have=0, room=1 << 30):
    """random literals and matches within the window; have: bytes of the member in front.  -> tokens, bytes they make"""
    alphabet = [int(x) for x in rng.integers(0, 256, size=int(rng.integers(1, 80)))]
    toks, n = [], 0
    p_match = (0.0, 0.1, 0.4, 0.8)[int(rng.integers(0, 4))]
    u = rng.random(size=(ntok, 2))
    r = rng.integers(0, 1 << 30, size=(ntok, 4)).tolist()
    for i in range(ntok):
        if have + n > 0 and u[i, 0] < p_match:
            length = (3, 4, 10, 257, 258, 3 + r[i][0] % 256)[r[i][1] % 6]
            far = min(have + n, 32768)
            dist = min((1, 2, far, 1 + r[i][2] % far, 1 + r[i][2] % min(far, 300))[r[i][3] % 5], far)
            if n + length > room:
                break
            toks.append((length, dist, True) if length == 258 and u[i, 1] < 0.5 else (length, dist))
            n += length
        else:
            if n + 1 > room:
                break
            toks.append(alphabet[r[i][0] % len(alphabet)])
            n += 1
    return toks, n


def _used_symbols(tokens):
    lits, dists = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(length_symbol(t[0], len(t) > 2 and t[2])[0])
            dists.add(distance_symbol(t[1])[0])
    return lits, dists


def random_dynamic(rng, s, tokens, final):
    """a dynamic block for the tokens: random valid codes (complete, or the single-code cases), a random header coding"""
    lits, dists = _used_symbols(tokens)
    nl_max = int(rng.integers(max(lits) + 1, 287)) if rng.random() < 0.5 else max(max(lits) + 1, 257)
    spare = [x for x in range(nl_max) if x not in lits]
    extra = [int(x) for x in rng.permutation(spare)[: int(rng.integers(0, 20))]] if spare else []
    ls = sorted(lits) + extra
    if len(ls) == 1:
        lit_lens = spread(286, ls, [1])  # the end-of-block symbol alone, one bit
    else:
        lit_lens = spread(286, ls, random_code(rng, len(ls), 15))
    nd_max = int(rng.integers(max(dists, default=0) + 1, 31))
    spare = [x for x in range(nd_max) if x not in dists]
    extra = [int(x) for x in rng.permutation(spare)[: int(rng.integers(0, 6))]] if spare else []
    ds = sorted(dists) + extra
    if len(ds) == 0:
        dist_lens = [0]
    elif len(ds) == 1:
        dist_lens = spread(30, ds, [1])  # one code of one bit (as libdeflate writes it)
    else:
        dist_lens = spread(30, ds, random_code(rng, len(ds), 15))
    hlit = int(rng.integers(max([257] + [i + 1 for i, l in enumerate(lit_lens) if l]), 287))
    hdist = int(rng.integers(max([1] + [i + 1 for i, l in enumerate(dist_lens) if l]), 31))
    if rng.random() < 0.5:
        hlit = max([257] + [i + 1 for i, l in enumerate(lit_lens) if l])
        hdist = max([1] + [i + 1 for i, l in enumerate(dist_lens) if l])
    lens = (lit_lens + [0] * hlit)[:hlit] + (dist_lens + [0] * hdist)[:hdist]
    cl_syms = rle_random(rng, lens) if rng.random() < 0.8 else rle_greedy(lens)
    used = sorted({x for x, _ in cl_syms})
    spare = [x for x in range(19) if x not in used]
    used += [int(x) for x in rng.permutation(spare)[: int(rng.integers(0 if len(used) > 1 else 1, 4))]]
    cl_lens = spread(19, used, random_code(rng, len(used), 7))
    hclen = int(rng.integers(max([4] + [i + 1 for i, x in enumerate(CL_ORDER) if cl_lens[x]]), 20))
    s.dynamic(tokens, lit_lens, dist_lens, final=final, hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, cl_syms=cl_syms)


def random_raw(rng, room=1 << 30, max_tokens=1000):
    """one random legal raw stream of at most `room` bytes of text -> Stream"""
    s = Stream()
    nblocks = int(rng.integers(1, 7))
    n = 0
    for b in range(nblocks):
        final = b == nblocks - 1
        kind = int(rng.integers(0, 4))
        if kind == 0:
            data = rng.integers(0, 256, size=min(int(rng.choice([0, 1, 100, 2000])), room - n), dtype=np.uint8).tobytes()
            s.stored(data, final, pad_bits=int(rng.integers(0, 256)))
            n += len(data)
            continue
        toks, k = random_tokens(rng, int(rng.choice([0, 1, 5, 300, max_tokens])), n, room - n)
        n += k
        if kind == 1:
            s.fixed(toks, final)
        else:
            random_dynamic(rng, s, toks, final)
    return s


def random_gz(rng, max_tokens=1000):
    """a random legal file in a random wrapper -> (bytes, text, members, is BGZF)"""
    wrap = int(rng.integers(0, 4))
    if wrap == 3:  # BGZF
        parts = [random_raw(rng, 65536, min(max_tokens, 3000)) for _ in range(int(rng.integers(1, 5)))]
        blocks = [(p.raw(), p.data()) for p in parts]
        eof = bool(rng.random() < 0.7)
        return bgzf(blocks, eof), b"".join(d for _, d in blocks), len(blocks) + eof, True
    out, text = [], []
    nmem = 1 if wrap == 0 else int(rng.integers(1, 4))
    for _ in range(nmem):
        p = random_raw(rng, 1 << 30, max_tokens)
        d = p.data()
        kw = {}
        if rng.random() < 0.3:
            kw["extra"] = rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        if rng.random() < 0.3:
            kw["name"] = b"reads_%d.fq" % int(rng.integers(0, 100))
        if rng.random() < 0.2:
            kw["comment"] = b"written by nobody"
        if rng.random() < 0.2:
            kw["hcrc"] = True
        out.append(gzip_member(p.raw(), d, **kw))
        text.append(d)
    return b"".join(out), b"".join(text), nmem, False


# ---- the corpus ----
def _noise(rng, n, alphabet=None):
    if alphabet is None:
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=n))


ALPHA62 = bytes(range(48, 58)) + bytes(range(65, 91)) + bytes(range(97, 123))
# 62 literals, the end of block and length symbol 257 (length 3): 64 codes of 6 bits
LIT64 = spread(258, list(ALPHA62) + [256, 257], [6] * 64)


def nonstrict_stream(rng, nblocks, lits_per_block):
    """Every dynamic header legal, none as an encoder writes it: all 286 + 30 lengths sent (the last of either list zero) and all 19 lengths of
    the code-length code (the last, symbol 15's, zero).  The block-start finder's strict rule refuses every one of them."""
    s = Stream()
    dist_lens = spread(30, [0, 28], [1, 1])
    for b in range(nblocks):
        toks = [_noise(rng, lits_per_block, ALPHA62), (3, 1), (3, int(rng.integers(16385, 16385 + 8192)) if b > 3 else 1)]
        lens = LIT64 + [0] * (286 - len(LIT64)) + dist_lens
        cl_syms = rle_greedy(lens)
        used = sorted({x for x, _ in cl_syms})
        s.dynamic(toks, LIT64, dist_lens, final=b == nblocks - 1, hlit=286, hdist=30, hclen=19, cl_lens=spread(19, used, flat_code(len(used))), cl_syms=cl_syms)
    return s


def corpus(seed=20240607, nrandom=200):
    """-> [Entry]: the named cases and `nrandom` random legal streams.  Every entry has been put to both references (zlib's inflater and
    expand); an entry with want = None is one zlib refuses."""
    rng = np.random.default_rng(seed)
    E = []

    def legal(what, s, **kw):
        d = s.data()
        E.append(_check(what, gzip_member(s.raw(), d, **kw), d))

    def illegal(what, s):
        E.append(_check(what, gzip_member(s.raw(), s.data(tolerant=True)), None))
    pre = _noise(rng, 32768)
    half = pre[:16384]

    # -- distances
    toks = [pre]
    for ds in range(30):
        toks += [("sym", 257, 0, ds, 0), ("sym", 258, 0, ds, (1 << DIST_EXTRA[ds]) - 1), 7]
    legal("every distance symbol, smallest and largest extra bits (fixed)", Stream().fixed(toks, True))
    for d in (32506, 32507, 32767, 32768):
        legal("distance %d" % d, Stream().fixed([pre, (3, d), (258, d), (258, d, True), 9, (17, d)], True))
    for n in (1, 2, 257, 4096, 32768):
        legal("distance = the %d bytes there are" % n, Stream().fixed([pre[:n], (258, n)], True))
        if n < 32768:
            illegal("distance one more than the %d bytes there are" % n, Stream().fixed([pre[:n], (258, n + 1)], True))
    illegal("a match as the first symbol", Stream().fixed([(3, 1)], True))
    illegal("too far, dynamic block, after a stored block", Stream().stored(pre[:100]).dynamic([65, (5, 102)], spread(260, [65, 256, 259], [1, 2, 2]), spread(14, [13], [1]), True))
    first = Stream().fixed([pre[:20000], (258, 20000), half], True)
    for tag, d, ok in (("exactly the member's bytes", 10, True), ("into the previous member", 11, False), ("far into the previous member", 32768, False)):
        second = Stream().fixed([half[:10], (100, d), 5], True)
        d1 = first.data()
        d2 = second.data() if ok else second.data(history=d1, tolerant=True)
        blob = gzip_member(first.raw(), d1) + gzip_member(second.raw(), d2)
        E.append(_check("second member, distance " + tag, blob, d1 + d2 if ok else None, 2))
        blob = bgzf([(first.raw(), d1), (second.raw(), d2)])
        E.append(_check("second BGZF block, distance " + tag, blob, d1 + d2 if ok else None, 3, True))
    toks = [b"abcdefgh"]
    for d in range(1, 9):
        for l in (3, 4, 7, 8, 9, 15, 16, 17, 31, 63, 64, 65, 129, 257, 258):
            toks += [(l, d), 48 + d]
    legal("copies of distance 1 to 8, lengths up to 258", Stream().fixed(toks, True))
    for L in (16, 7, 1, 258):
        legal("255 matches, each a copy of the one before (%d bytes each)" % L, Stream().fixed([pre[:L]] + [(max(L, 3), L)] * 255, True))
    toks = [pre[:300]]
    for off in range(0, 260, 13):  # the long matches are more than a batch's bytes: its last one ends 0 .. 258 bytes short of the boundary
        toks += [_noise(rng, off, ALPHA62)] + [(258, 300), (258, 1, True)] * (kBatchBytes // 516 + 2)
    legal("length-258 matches around the boundary of the %d-byte batch" % kBatchBytes, Stream().fixed(toks, True))
    toks = [pre[:300]]
    for off in range(kBatchSyms - 156, kBatchSyms + 44, 9):  # literals fill the batch's symbols, the long matches stand where it has to end
        toks += [_noise(rng, off, ALPHA62), (258, 300), (258, 1, True), (258, 258)]
    legal("length-258 matches around the boundary of the %d-symbol batch" % kBatchSyms, Stream().fixed(toks, True))
    # a job that starts inside the stream (the finder enters at a block start as encoders write it) and copies from the 32 KB in front of it:
    # window symbols 0x8000 + 0 and 0x8000 + 32767
    s = Stream()
    lens62 = spread(286, list(ALPHA62) + [256, 257, 285], [6] * 63 + [7, 7])
    d2 = spread(30, [0, 29], [1, 1])
    s.dynamic([_noise(rng, 40000, ALPHA62)], lens62, d2)
    for first_tok in ((3, 32768), (3, 1), (258, 32768), (258, 32767)):
        s.dynamic([first_tok, _noise(rng, 14000, ALPHA62), (258, 1)], lens62, d2)
    s.dynamic([(3, 32768), b"end"], lens62, d2, True)
    legal("jobs entered at a block whose first symbol copies window bytes 0 and 32767", s)

    # -- lengths
    toks = [pre[:600]]
    for ls in range(257, 286):
        toks += [("sym", ls, 0, 0, 0), ("sym", ls, (1 << LEN_EXTRA[ls - 257]) - 1, 17, 3), 33]
    legal("every length symbol, smallest and largest extra bits", Stream().fixed(toks, True))
    legal("length 258 both ways", Stream().fixed([b"xy", (258, 2), (258, 2, True), ("sym", 285, 0, 1, 0), ("sym", 284, 31, 1, 0)], True))

    # -- code shapes
    syms = list(range(65, 80)) + [256]
    ll = spread(257, syms, list(range(1, 16)) + [15])
    legal("a literal/length code of every length 1 to 15", Stream().dynamic([bytes(rng.choice(syms[:15], size=3000).astype(np.uint8))], ll, [0], True))
    syms = list(range(65, 75)) + [97, 98, 99, 100, 257, 256]  # ten rare symbols of 1 .. 10 bits, then 11 12 13 14 15 15
    ll = spread(258, syms, list(range(1, 11)) + [11, 12, 13, 14, 15, 15])
    toks = [b"abcd"]
    for _ in range(600):
        toks += [bytes(rng.choice([97, 98, 99, 100], size=int(rng.integers(1, 30))).astype(np.uint8)), (3, int(rng.integers(1, 5)))]
    legal("frequent symbols with codes of 11 to 15 bits", Stream().dynamic(toks + [65, 74], ll, spread(4, [0, 1, 2, 3], [2, 2, 2, 2]), True))
    dsyms = list(range(0, 8)) + list(range(14, 22))  # eight rare ones of 1 .. 8 bits, then 9 .. 15, 15
    dl = spread(30, dsyms, list(range(1, 9)) + list(range(9, 16)) + [15])
    toks = [pre[:2100]]
    for _ in range(1500):
        ds = int(rng.choice(dsyms[8:]))
        toks += [("sym", 257 + int(rng.integers(0, 8)), 0, ds, int(rng.integers(0, 1 << DIST_EXTRA[ds]))), int(rng.integers(65, 70))]
    toks += [("sym", 257, 0, ds, 0) for ds in dsyms[:8]]
    ll = spread(265, list(range(256)) + list(range(256, 265)), flat_code(265))
    legal("distance codes of 9 to 15 bits", Stream().dynamic(toks, ll, dl, True))
    ll = spread(258, [65, 67, 257, 256, 71], [1, 2, 3, 4, 4])
    toks = [b"ACGAAC"]
    for _ in range(800):
        toks += [bytes(rng.choice([65, 67, 71], size=int(rng.integers(0, 9)), p=[.6, .3, .1]).astype(np.uint8)), ("sym", 257, 0, int(rng.integers(0, 3)), 0)]
    legal("literal codes of 1 to 4 bits, distance codes of 1 and 2 bits", Stream().dynamic(toks, ll, [1, 2, 2], True))
    toks = [bytes(range(256)) * 2]
    for i, ls in enumerate(list(range(257, 286)) + [257]):
        toks += [("sym", ls, 0, i, 0)]
    legal("all 286 literal/length and all 30 distance symbols in use", Stream().stored(pre).dynamic(toks, flat_code(286), flat_code(30), True))
    one = spread(30, [5], [1])
    ll = spread(259, [65, 66, 256, 257, 258], [2, 2, 2, 3, 3])
    legal("one distance code of one bit: matches through it", Stream().dynamic([b"ABBABABA", (3, 7), (4, 8), 65, (3, 7)], ll, one, True))
    legal("one distance code of one bit: distance symbol 0", Stream().dynamic([b"AB", (4, 1), (3, 1)], ll, [1], True))
    illegal("one distance code of one bit: the unassigned bit pattern", Stream().dynamic([b"ABBABABA", ("sym", 257, 0, None, 0), ("bits", 1, 1), 65], ll, one, True))
    legal("no distance code: all literals", Stream().dynamic([b"ABBA" * 50], ll, [0], True))
    illegal("no distance code: a match", Stream().dynamic([b"ABBA", ("sym", 257, 0, None, 0), ("bits", 0, 1), 65, 66], ll, [0], True))
    legal("only the end-of-block symbol, one bit, in an empty dynamic block", Stream().dynamic([], spread(257, [256], [1]), [0], True))
    legal("an empty dynamic block in front of text", Stream().dynamic([], spread(257, [256], [1]), [0]).fixed([b"text"], True))
    for ls in (286, 287):
        illegal("fixed block, literal/length symbol %d" % ls, Stream().fixed([b"abc", ("sym", ls, 0, None, 0), 65, 66, 67], True))
    for ds in (30, 31):
        illegal("fixed block, distance symbol %d" % ds, Stream().fixed([b"abc", ("sym", 257, 0, ds, 0), 65, 66, 67], True))

    # -- headers
    ll = spread(286, list(range(60, 70)) + list(range(276, 286)) + [256, 257], [5] * 20 + [3, 2])  # the literal/length lengths end ... 5 5 5 5
    dl = [5, 5, 5, 5] + [0] * 18 + [3, 3, 3, 2, 2]
    lens = ll + dl
    at = 286 - 3
    cl_syms = rle_greedy(lens[:at]) + [(16, 3)] + rle_greedy(lens[at + 6:])  # five 5s, repeated six times: across the seam
    legal("a run of symbol 16 that crosses from the literal/length into the distance lengths",
          Stream().stored(pre[:9000]).dynamic([b"<=>?@ABCDE", (3, 2), ("sym", 276, 0, 0, 0), ("sym", 285, 0, 26, 0)], ll, dl, True, cl_syms=cl_syms))
    ll0 = spread(270, [65, 66, 256, 257], [1, 2, 3, 3])
    dl0 = [0] * 20 + [1]
    cl_syms = rle_greedy(ll0[:258]) + [(18, 286 - 258 + 20 - 11)] + [(1, 0)]
    legal("a run of symbol 18 that crosses from the literal/length into the distance lengths",
          Stream().stored(pre[:2000]).dynamic([b"ABBA", (3, 1025)], ll0, dl0, True, hlit=286, hdist=21, cl_syms=cl_syms))
    good_l, good_d = spread(258, [65, 66, 256, 257], [2, 2, 2, 2]), [1, 1]
    lens = good_l + good_d
    illegal("symbol 16 as the first code-length symbol", Stream().dynamic([65], good_l, good_d, True, cl_syms=[(16, 0)] + rle_none(lens[3:])))
    illegal("a run that passes the end of the length list", Stream().dynamic([65], good_l, good_d, True, cl_syms=rle_greedy(lens[:65]) + [(18, 127)] + rle_none(lens[65 + 138:]) + [(17, 7)]))
    illegal("a run of symbol 16 that passes the end of the length list", Stream().dynamic([65], good_l, good_d, True, cl_syms=rle_greedy(lens[:-1]) + [(16, 3)]))
    cl = rle_greedy(lens)
    used = sorted({x for x, _ in cl})
    assert 3 <= len(used) < 8
    illegal("an incomplete code-length code", Stream().dynamic([65], good_l, good_d, True, cl_syms=cl, cl_lens=spread(19, used, [3] * len(used))))
    illegal("an over-subscribed code-length code", Stream().dynamic([65], good_l, good_d, True, cl_syms=cl, cl_lens=spread(19, used, [1] * len(used))))
    illegal("no end-of-block symbol", Stream().dynamic([65, 66], spread(258, [65, 66, 255, 257], [2, 2, 2, 2]), good_d, True, eob=False))
    illegal("an over-subscribed literal/length code", Stream().dynamic([65], spread(258, [65, 66, 67, 256, 257], [2, 2, 2, 2, 2]), good_d, True))
    illegal("an incomplete literal/length code", Stream().dynamic([65], spread(258, [65, 66, 256], [2, 2, 2]), good_d, True))
    illegal("an incomplete distance code of two symbols", Stream().dynamic([65], good_l, [2, 2], True))
    illegal("an incomplete distance code: one symbol of two bits", Stream().dynamic([65], good_l, [2], True))
    illegal("an over-subscribed distance code", Stream().dynamic([65], good_l, [1, 1, 1], True))
    for hlit in (287, 288):
        illegal("HLIT %d" % (hlit - 257), Stream().dynamic([65], good_l, good_d, True, hlit=hlit))
    for hdist in (31, 32):
        illegal("HDIST %d" % (hdist - 1), Stream().dynamic([65], good_l, good_d, True, hdist=hdist))
    illegal("block type 3", Stream().block3(True))
    illegal("block type 3 after a good block", Stream().fixed([b"good"]).block3(True))
    legal("legal headers no encoder writes, megabytes of them (the finder's second pass)", nonstrict_stream(rng, 420, 6500))

    # -- block structure
    s = Stream()
    seen = set()
    for j in range(8):
        s.fixed([200] * j)  # (a 9-bit literal each: the stored block's header starts at every bit of a byte)
        seen.add(s.w.nbits % 8)
        s.stored(_noise(rng, 100 + j), pad_bits=0xff)
    assert len(seen) == 8
    legal("stored blocks at all eight bit alignments, padding bits set", s.stored(b"", True, pad_bits=0x55))
    legal("stored blocks of 0 and 65535 bytes", Stream().stored(b"").stored(_noise(rng, 65535)).stored(b"").stored(b"tail", True))
    illegal("a stored block with a bad NLEN", Stream().stored(b"stored data", True, nlen=(11 ^ 0xffff) ^ 0x100))
    illegal("a stored block with a bad NLEN after text", Stream().fixed([pre[:5000]]).stored(b"stored data", True, nlen=11))
    s = Stream()
    for _ in range(1000):
        s.fixed([])
    legal("a thousand empty fixed blocks", s.fixed([b"after"], True))
    s = Stream()
    for i in range(1000):
        c = 33 + i % 90
        s.dynamic([c], spread(257, [c, 256], [1, 1]), [0])
    legal("a thousand dynamic blocks of one symbol", s.dynamic([10], spread(257, [10, 256], [1, 1]), [0], True))
    toks = []
    for i in range(100):
        toks += [_noise(rng, 9990, ALPHA62), (3, 1)] + ([(3, 32768), (3, 29000)] if i > 3 else [(3, 1), (3, 1)]) + [48] * 7
    assert sum(len(t) if isinstance(t, bytes) else 1 for t in toks) == 1_000_000
    legal("one dynamic block of a million symbols", Stream().dynamic(toks, LIT64, spread(30, [0, 29], [1, 1]), True))
    s = Stream()
    for i in range(36):
        s.stored(_noise(rng, 65535, b"ACGT\n"), pad_bits=i)
        t, _ = random_tokens(rng, 1000, 65535)
        s.fixed(t)
    legal("megabytes of fixed and stored blocks only", s.fixed([(258, 32768)], True))
    legal("a final stored block at the start", Stream().stored(b"stored", True))
    legal("a final fixed block at the start", Stream().fixed([b"fixed", (5, 5)], True))
    legal("a final dynamic block at the start", Stream().dynamic([b"ABBA", (3, 2)], good_l, good_d, True))
    legal("header fields", Stream().fixed([b"fields"], True), extra=b"\x05\0hello", name=b"name.fq", comment=b"a comment", hcrc=True)

    # -- false starts: a whole .gz of many dynamic blocks as the payload of stored blocks
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 1)  # memLevel 1: a block every few hundred symbols
    inner = co.compress(_noise(rng, 600_000, b"ACGTACGTACGTN\n")) + co.flush()
    s = Stream().fixed([b"in front"])
    for a in range(0, len(inner), 50001):
        s.stored(inner[a:a + 50001], pad_bits=a & 0xff)
    legal("a whole .gz carried in stored blocks: every block start in it is a false one", s.dynamic([b"ABBA", (3, 32768)], good_l, spread(30, [29, 0], [1, 1]), True))

    # -- random legal streams
    for i in range(nrandom):
        blob, text, members, is_bgzf = random_gz(rng)
        E.append(_check("random %d" % i, blob, text, members, is_bgzf))
    return E


def bgzf_forms(entries):
    """Every single-member entry small enough for a BGZF block, as a BGZF file: its stream in the first block (a `BC` field, a job that
    decodes one member), a block of text behind it, the EOF block.  An illegal stream makes an illegal file."""
    out = []
    tail = Stream().fixed([b"the block behind\n"], True)
    for e in entries:
        if e.members != 1 or e.bgzf or (e.want is not None and len(e.want) > 65536):
            continue
        flg = e.blob[3]
        at = 10
        if flg & 4:
            at += 2 + struct.unpack_from("<H", e.blob, at)[0]
        for f in (8, 16):
            if flg & f:
                at = e.blob.index(b"\0", at) + 1
        at += 2 if flg & 2 else 0
        raw = e.blob[at:-8]
        if len(raw) + 26 > 65536:
            continue
        isize = struct.unpack_from("<I", e.blob, len(e.blob) - 4)[0]
        if isize > 65536:
            continue
        blob = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw + e.blob[-8:] + bgzf([(tail.raw(), tail.data())])
        out.append(_check("BGZF: " + e.name, blob, None if e.want is None else e.want + tail.data(), 3, True))
    return out
