"""Shared helpers for the parity tests (synthetic reads / genomes; not product code)."""
import numpy as np


def random_genomes(rng, ngenomes, length, with_n=False):
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=ngenomes * length).astype(np.uint8)
    if with_n:
        idx = rng.integers(0, bases.size, size=max(bases.size // 500, 1))
        bases[idx] = ord("N")
    offsets = (np.arange(ngenomes + 1, dtype=np.uint64) * np.uint64(length))
    return bases, offsets


_COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[a] = b


def sample_reads(rng, gbases, goffsets, nreads, readlen, err=0.01, ragged=False, lower=False, present=None):
    """Reads drawn from genomes (both strands, substitution errors). -> (bases u8, offsets u64, source genome)."""
    g = len(goffsets) - 1
    present = np.arange(g) if present is None else np.asarray(present)
    src = present[rng.integers(0, len(present), size=nreads)]
    lens = np.full(nreads, readlen, dtype=np.int64)
    if ragged:
        lens = rng.integers(max(readlen // 3, 1), readlen + 1, size=nreads)
    glen = (goffsets[1:] - goffsets[:-1]).astype(np.int64)
    start = (rng.random(nreads) * np.maximum(glen[src] - lens, 1)).astype(np.int64) + goffsets[src].astype(np.int64)
    offsets = np.zeros(nreads + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    out = np.empty(int(offsets[-1]), dtype=np.uint8)
    rev = rng.random(nreads) < 0.5
    for i in range(nreads):
        s = gbases[start[i]: start[i] + lens[i]]
        if rev[i]:
            s = _COMP[s[::-1]]
        out[int(offsets[i]): int(offsets[i + 1])] = s
    if err > 0:
        m = rng.random(out.size) < err
        out[m] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(m.sum()))
    if lower:
        m = rng.random(out.size) < 0.1
        out[m] = out[m] | 0x20
    return out, offsets, src


def job_sketch_size(oracle, job, ki, bases, offsets, k, table_hashes, s=0):
    """How many hashes the read sketch of a ShardJob holds for its k number ki: what passes the table's bit filter — or, when
    the job has built the table's resident index (dense tables, s = 0), exactly the read k-mers that are hashes of the table."""
    filt = job.engine.filters[ki] if ki < len(job.engine.filters) else None
    hmax = int(table_hashes.max())
    if s == 0 and filt is not None and filt.resident_bytes > 0:
        h = oracle.sketch_reads(bases, offsets, k, hmax=hmax)[0]
        return int(np.isin(h, table_hashes).sum())
    return len(oracle.sketch_reads_filtered(bases, offsets, k, table_hashes, hmax=hmax, s=s)[0])


def flat(seqs):
    """list of bytes -> (bases u8, offsets u64)"""
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offs


def refpipe_case(rng, ngenomes=5, glen=(1200, 2000), nreads=60, strains=True):
    """Genomes that SHARE k-mers (a strain = a mutated copy; repeats inside one genome; a reverse-complemented copy), N runs,
    lower case, degenerate genomes; reads from three of them, both strands, each twice so that ci = 2 is met, plus noise.
    -> (genomes: list of bytes, reads: list of bytes)"""
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rand(n, lo, hi, p_n=0.002, p_lower=0.05):
        out = []
        for _ in range(n):
            ln = int(rng.integers(lo, hi + 1))
            b = rng.choice(alpha, size=ln).astype(np.uint8)
            b[rng.random(ln) < p_n] = ord("N")
            m = rng.random(ln) < p_lower
            b[m] |= 0x20
            out.append(b.tobytes())
        return out
    genomes = rand(ngenomes, *glen)
    if strains:
        g0 = bytearray(genomes[0].upper())
        for p in rng.integers(0, len(g0), size=12):
            g0[int(p)] = b"ACGT"[int(rng.integers(0, 4))]
        genomes.append(bytes(g0))
        genomes.append(genomes[1][:600] + genomes[1][100:700])
        genomes.append(genomes[2].upper().translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])
    genomes += [b"ACGT" * 5, b"", b"A" * 300]
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads = []
    for g in (0, 2, 4):
        src = genomes[g]
        for _ in range(nreads):
            a = int(rng.integers(0, max(len(src) - 150, 1)))
            r = src[a:a + 150]
            if rng.random() < 0.5:
                r = r.translate(comp)[::-1]
            reads += [r, r]
    reads += rand(40, 60, 150, p_n=0.01, p_lower=0.1) + [b"", b"ACG"]
    return genomes, reads


# ---- reads built tile by tile: the persistent stage-A kernels take 64 reads to a wavefront and loop over tiles, so what one tile
# leaves behind (staged bases, not-a-base bits, walk mode, run lists, candidate buffer, totals) meets the next tile of a DIFFERENT kind
TILE = 64
TILE_KINDS = ("clean", "ragged", "bad", "long", "span", "short", "foreign", "repeat")
_TILE_WEIGHTS = (0.3, 0.1, 0.12, 0.06, 0.06, 0.1, 0.1, 0.12)
# what the tests want some wavefront to walk one right after the other: a clean tile behind every kind that leaves state behind
# (not-a-base bits, a chunked walk, a skipped tile, full run lists, a gate that rejected everything), and every other walk behind a clean one
TILE_TRANSITIONS = ({(a, "clean") for a in ("bad", "long", "span", "short", "foreign", "repeat", "ragged")}
                    | {("clean", b) for b in ("bad", "long", "span", "short", "ragged")})
_IUPAC = np.frombuffer(b"RYKMSWBDHVN", dtype=np.uint8)


def tile_genomes(rng, ngenomes=12, length=20000):
    """Genomes for tile_sample: random bases; genome 0 carries a homopolymer and tandem repeats of short units from 1000 on.
    -> (bases u8, offsets u64)"""
    gb, go = random_genomes(rng, ngenomes, length)
    rep = b"A" * 300 + b"ACGTTGA" * 40 + b"C" * 200 + b"AC" * 150 + b"GATTACAGATTACAT" * 20
    gb[1000:1000 + len(rep)] = np.frombuffer(rep, dtype=np.uint8)
    return gb, go


def tile_kinds(rng, ntiles):
    """A kind of TILE_KINDS for every tile, at random, every kind at least twice."""
    kinds = list(rng.choice(len(TILE_KINDS), size=ntiles, p=np.array(_TILE_WEIGHTS) / sum(_TILE_WEIGHTS)))
    for i in range(len(TILE_KINDS)):
        if kinds.count(i) < 2:
            kinds[int(rng.integers(0, ntiles))] = i
            kinds[int(rng.integers(0, ntiles))] = i
    return [TILE_KINDS[i] for i in kinds]


def tile_sample(rng, gbases, goffsets, kinds, k, last=TILE, main=0, present=(0, 1, 2, 3, 4, 5)):
    """64 reads of kinds[t] for tile t (`last` reads in the final one), both strands, 1 % substitutions:
      clean    equal 150 bp reads, half of them from genome `main` (high coverage), the rest from `present`
      ragged   k - 1 .. 250 bp
      bad      150 bp with N runs, lower case and IUPAC letters
      long     150 bp and one read of 1100-3000 bp, one of exactly 1023 and one of 1024 (the chunked path of k_count_kmers)
      span     400-1000 bp: no read above 1023, the tile's span above any stage sized by a batch's average
      short    0 .. k - 1 bp: no window in the tile
      foreign  150 bp of random bases (no genome's)
      repeat   homopolymers, tandem repeats of 1-12 bp units, reads of genome 0's repeats
    -> (bases u8, offsets u64) of len(kinds) tiles"""
    alpha = np.frombuffer(b"ACGT", dtype=np.uint8)
    glen = (goffsets[1:] - goffsets[:-1]).astype(np.int64)
    present = np.asarray(present)

    def from_genome(n):
        g = int(main) if rng.random() < 0.5 else int(present[rng.integers(0, len(present))])
        n = min(n, int(glen[g]))
        a = int(goffsets[g]) + int(rng.integers(0, int(glen[g]) - n + 1))
        s = gbases[a:a + n].copy()
        if rng.random() < 0.5:
            s = _COMP[s[::-1]]
        m = rng.random(n) < 0.01
        s[m] = rng.choice(alpha, size=int(m.sum()))
        return s

    reads = []
    for t, kind in enumerate(kinds):
        nr = last if t == len(kinds) - 1 else TILE
        if kind == "clean":
            tile = [from_genome(150) for _ in range(nr)]
        elif kind == "ragged":
            tile = [from_genome(int(n)) for n in rng.integers(max(k - 1, 0), 251, size=nr)]
        elif kind == "bad":
            tile = []
            for _ in range(nr):
                s = from_genome(150)
                if rng.random() < 0.5:
                    a = int(rng.integers(0, 150))
                    s[a:a + int(rng.integers(1, 21))] = ord("N")
                m = rng.random(150) < 0.005
                s[m] = rng.choice(_IUPAC, size=int(m.sum()))
                m = rng.random(150) < 0.1
                s[m] |= 0x20
                tile.append(s)
        elif kind == "long":
            tile = [from_genome(150) for _ in range(nr)]
            for i, n in zip(rng.permutation(nr)[:3], (int(rng.integers(1100, 3001)), 1023, 1024)):
                tile[i] = from_genome(n)
        elif kind == "span":
            tile = [from_genome(int(n)) for n in rng.integers(400, 1001, size=nr)]
        elif kind == "short":
            tile = [from_genome(int(n)) if n else np.zeros(0, np.uint8) for n in rng.integers(0, max(k, 1), size=nr)]
        elif kind == "foreign":
            tile = [rng.choice(alpha, size=150).astype(np.uint8) for _ in range(nr)]
        elif kind == "repeat":
            tile = []
            for _ in range(nr):
                r = rng.random()
                if r < 0.3:
                    s = np.full(150, alpha[int(rng.integers(0, 4))], dtype=np.uint8)
                elif r < 0.6:
                    unit = rng.choice(alpha, size=int(rng.integers(1, 13))).astype(np.uint8)
                    s = np.tile(unit, 150 // len(unit) + 1)[:150]
                else:
                    a = 1000 + int(rng.integers(0, 1100))
                    s = gbases[a:a + 150].copy()
                tile.append(s)
        else:
            raise ValueError(kind)
        reads += tile
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    return (np.concatenate(reads).astype(np.uint8) if reads else np.zeros(0, np.uint8)), offsets


def wave_tiles(ntiles, grid, waves=4):
    """The tiles every wavefront of a persistent grid of `grid` workgroups of `waves` wavefronts walks, in its order: wavefront w
    takes tiles w, w + waves * grid, ... (tile % (waves * grid) == w).  -> [[tile, ...] per wavefront]"""
    n = waves * grid
    return [list(range(w, ntiles, n)) for w in range(min(n, ntiles))]


def tile_transitions(kinds, grid, waves=4):
    """{(kind, next kind)}: the pairs of tiles some wavefront walks one right after the other at this grid."""
    out = set()
    for seq in wave_tiles(len(kinds), grid, waves):
        out.update((kinds[a], kinds[b]) for a, b in zip(seq, seq[1:]))
    return out


# ---- every k: the builders of tests/test_gpu_every_k.py (one small sample per k that reaches what changes with k)
def revcomp(s):
    """bytes -> the reverse complement (upper or lower case; N stays N)"""
    return bytes(_COMP[np.frombuffer(s, dtype=np.uint8)[::-1]])


def unpack_kmer(hi, lo, k):
    """A table's 2-bit packed k-mer (first base most significant) -> bytes"""
    v = (int(hi) << 64) | int(lo)
    return bytes(b"ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def pack_kmer(s):
    """bytes of ACGT -> (hi, lo) as sketch_genomes_kmers packs them"""
    v = 0
    for ch in s:
        v = (v << 2) | b"ACGT".index(ch)
    return v >> 64, v & 0xFFFFFFFFFFFFFFFF


def palindrome(rng, k):
    """A k-mer that is its own reverse complement (k even)."""
    half = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k // 2).astype(np.uint8).tobytes()
    return half + revcomp(half)


def with_entry(entries, g, kmer, h):
    """sketch_genomes_kmers' entries with one more in genome g — the k-mer `kmer` matched by hash h — at its place by hash (at the end of
    a genome whose hashes do not ascend: a forward-selected one), unless the genome holds it already.  -> the same four arrays"""
    hashes, khi, klo, offs = entries
    a, b = int(offs[g]), int(offs[g + 1])
    hi, lo = pack_kmer(kmer)
    if np.any((khi[a:b] == np.uint64(hi)) & (klo[a:b] == np.uint64(lo))):
        return entries
    at = a + int(np.searchsorted(hashes[a:b], np.uint64(h))) if b > a and np.all(hashes[a + 1:b] >= hashes[a:b - 1]) else b
    ins = lambda arr, v: np.insert(arr, at, np.uint64(v))  # noqa: E731
    offs = offs.copy()
    offs[g + 1:] += np.uint64(1)
    return ins(hashes, h), ins(khi, hi), ins(klo, lo), offs


# the order of tiles that walks every pair of TILE_TRANSITIONS: a clean tile around every other kind
_KIND_CHAIN = ("clean", "bad", "clean", "long", "clean", "span", "clean", "short", "clean", "ragged", "clean", "foreign", "clean", "repeat", "clean")


def tile_kinds_walked(rng, ntiles, grid=1, waves=4, seg=5):
    """tile_kinds, with the first `seg` tiles of the wavefronts of a persistent grid of `grid` workgroups laid out so that together they
    walk _KIND_CHAIN (each wavefront's piece begins with the kind the last one's ended on): every kind, every pair of TILE_TRANSITIONS.
    Needs seg tiles on enough wavefronts: ntiles >= 4 * seg at grid 1."""
    kinds = tile_kinds(rng, ntiles)
    pos = 0
    for seq in wave_tiles(ntiles, grid, waves):
        if pos >= len(_KIND_CHAIN) - 1:
            break
        for t, kind in zip(seq, _KIND_CHAIN[pos:pos + seg]):
            kinds[t] = kind
        pos += seg - 1
    return kinds


def edge_reads(rng, gbases, goffsets, k, table_kmers, pal=None):
    """The reads at the edges of k: reads of k - 1, k and k + 1 bases of table k-mers; reads whose first and last windows are table
    k-mers, in both orientations and twice; reads of 1023, 1024, 1025 and 2600 bases (k_count_kmers takes reads above 1023 in chunks that
    overlap by k - 1); reads holding `pal` (a reverse-palindromic k-mer) and `pal` alone.  -> [bytes]"""
    g = bytes(gbases[int(goffsets[1]):int(goffsets[2])])
    out = []
    for i in range(3):
        a, b = table_kmers[(2 * i) % len(table_kmers)], table_kmers[(2 * i + 1) % len(table_kmers)]
        out += [a[:k - 1], a, a + b"ACGT"[i:i + 1], revcomp(b)]
        s = int(rng.integers(0, len(g) - 60))
        r = a + g[s:s + 20 + 13 * i] + b
        out += [r, revcomp(r)] * 2
    for n in (1023, 1024, 1025, 2600):
        s = int(rng.integers(0, len(g) - n + 1))
        out.append(g[s:s + n] if n != 1024 else revcomp(g[s:s + n]))
    if pal is not None:
        for i in range(3):
            s = int(rng.integers(0, len(g) - 60))
            out.append(g[s:s + 7 + i] + pal + g[s + 30:s + 60])
        out.append(pal)
    return out


def edge_sample(rng, gbases, goffsets, kinds, k, edges, last=TILE, main=0, present=(0, 1, 2, 3, 4, 5)):
    """tile_sample of `kinds`, where a kind "edge" is a tile of the next 64 of `edges` (the last such tile filled up with 150-base reads of
    genome `main`).  -> (bases u8, offsets u64)"""
    reads, e = [], list(edges)
    for t, kind in enumerate(kinds):
        nr = last if t == len(kinds) - 1 else TILE
        if kind == "edge":
            tile, e = e[:nr], e[nr:]
            while len(tile) < nr:
                a = int(goffsets[main]) + int(rng.integers(0, int(goffsets[main + 1] - goffsets[main]) - 150))
                tile.append(bytes(gbases[a:a + 150]))
            reads += tile
        else:
            b, o = tile_sample(rng, gbases, goffsets, [kind], k, last=nr, main=main, present=present)
            reads += [bytes(b[int(o[i]):int(o[i + 1])]) for i in range(len(o) - 1)]
    assert not e, "more edge reads than edge tiles"
    return flat(reads)


# ---- stage C through the sharded C ABI (test_gpu_fullsize.py, test_gpu_profile_geometry.py)
def stage_c_sharded(hip, recs, ref2tax, ntax, cuts, pct_id=0.5, info=None, assign=False):
    """Run stage C as len(cuts)+1 shards through mg_profile_begin_dev / _commit_dev; -> same dict as profile_assign.
    info (a dict): gets 'maps' and 'groups', every shard's state_map() and ngroups as the map-only passes gave them BEFORE any
    commit.  assign: commit through mg_profile_commit_assign_dev; info['words'] = every shard's verdict words."""
    from metalign_amd import _hip
    from metalign_amd.distributed import compose_incoming
    bounds = [0] + list(cuts) + [len(recs)]
    d_r2t = hip.array(ref2tax)
    acc = hip.empty(3 * ntax + 2, np.uint64)
    host = np.zeros(3 * ntax + 2, dtype=np.uint64)
    host[2 * ntax:3 * ntax] = 0xFFFFFFFFFFFFFFFF
    acc.upload(host)
    shards, arrays = [], []
    for i in range(len(bounds) - 1):
        a, b = bounds[i], bounds[i + 1]
        has_look = b < len(recs)
        part = recs[a:b + (1 if has_look else 0)]
        d = hip.array(part if len(part) else np.zeros(1, _hip.REC_DTYPE))
        arrays.append(d)
        shards.append(hip.profile_begin_dev(d.ptr, b - a, has_look, d_r2t.ptr, len(ref2tax), ntax, pct_id))
    maps = [s.state_map() for s in shards]
    groups = [s.ngroups for s in shards]
    if info is not None:
        info.update(maps=maps, groups=groups, words=[])
    mm_all = []
    base = acc.ptr
    first_nonempty = next(i for i in range(len(shards)) if bounds[i + 1] > bounds[i])
    for i, s in enumerate(shards):
        args = (compose_incoming(maps, i), i == first_nonempty, sum(groups[:i]), base, base + 8 * ntax, base + 16 * ntax, base + 24 * ntax)
        if assign:
            d_words = hip.empty(max(2 * groups[i], 2), np.uint64)
            s.commit_assign(*args, d_words.ptr)
            if info is not None:
                info["words"].append(d_words.download()[:2 * groups[i]])
            d_words.free()
        else:
            s.commit(*args)
        mm_all.append(s.multimapped())
    out = acc.download()
    off = [np.zeros(1, np.uint64)]
    tot_e = 0
    for o, t, h, r in mm_all:
        off.append(o[1:] + np.uint64(tot_e))
        tot_e += len(t)
    res = dict(count=out[:ntax], bases=out[ntax:2 * ntax], first_seen=out[2 * ntax:3 * ntax], tot_rds=int(out[3 * ntax]),
               n_ambig=int(out[3 * ntax + 1]), mm_offsets=np.concatenate(off),
               mm_tax=np.concatenate([m[1] for m in mm_all]), mm_hitlen=np.concatenate([m[2] for m in mm_all]),
               mm_read=np.concatenate([m[3] for m in mm_all]))
    for s in shards:
        s.free()
    for d in arrays + [d_r2t, acc]:
        d.free()
    return res
