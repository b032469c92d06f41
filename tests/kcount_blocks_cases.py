"""The tiles that the walk in blocks of 32 candidates (mg_kcount_core.h: kc_walk32) is held to the oracle by, on the host
(test_kcount_blocks_host.py) and on the GPU (test_gpu_kcount_blocks.py): read lengths around the points where a block, a
stream dword or the tail block begins or ends, a base that is no base at the dword and block boundaries, and reads long enough
to fill a lane's list, so that the walk starts anew at windows that are no multiple of 16."""
import numpy as np

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
NGEN, GLEN = 6, 3000
KINDS = ("equal", "ragged", "equal_n", "ragged_n", "long", "long_equal", "long_equal_n")
LIST_CAP = 12     # slots of a lane's list in the kernel (mg_kcount.hip: kKcListCap)
STAGE_BASES = 16 * 2048  # the most a wavefront's stage holds (mg_count_kmers_dev): a tile above it is taken through in chunks


def cands(k):
    """candidates of a k-mer (mg_kcount_core.h: kc_cands)"""
    e = 2 + (k - 51) // 2 if k >= 53 else (2 if k >= 23 else (1 if k >= 19 else 0))
    return k - 14 - 2 * e


def must_restart(k, tile, cap=LIST_CAP):
    """A run is at most cands(k) windows long, so a read of more than cap * cands(k) windows closes more runs than a list of cap
    slots holds: the walk of its tile starts anew.  True when that holds for `tile` (64 reads) AND the tile fits the stage of a
    batch that is this tile alone (64 reads of average length + 12.5 %, capped) — the usual tile's path, not the chunked one."""
    lens = [len(r) for r in tile]
    avg = (sum(lens) + len(lens) - 1) // len(lens)
    sd = min(((64 * avg * 9 // 8 + 64 + 15) // 16 + 63) // 64 * 64, STAGE_BASES // 16)
    return max(lens) - k + 1 > cap * cands(k) and sum(lens) + 16 <= 16 * sd and max(lens) <= 1023


def genomes(rng):
    gs = [rng.choice(ALPHA, size=GLEN).astype(np.uint8) for _ in range(NGEN)]
    gs[1][500:520] = ord("A")  # a homopolymer: every m-mer of it is one value
    gs[2][100:160] = np.tile(np.frombuffer(b"ACGTTGCA", dtype=np.uint8), 8)[:60]  # a tandem repeat
    return gs


def lengths(k):
    return [k, k + 1, k + 30, k + 31, k + 32, k + 33, k + 63, k + 64, k + 65, 150]


def _read(rng, gs, L):
    g = int(rng.integers(0, NGEN))
    st = int(rng.integers(0, GLEN - L + 1))
    r = bytearray(gs[g][st:st + L])
    if rng.random() < 0.5:
        r = bytearray(bytes(r).translate(COMP)[::-1])
    for j in np.flatnonzero(rng.random(L) < 0.01):
        r[j] = int(rng.choice(ALPHA))
    return r


def reads(rng, gs, k, kind, tile=64, ls=None):
    """Tiles of `tile` reads each (a multiple of 64: a wavefront's tile is 64 reads).  equal: one tile per length of ls (lengths(k) unless given);
    ragged: four tiles with lengths drawn from them; *_n: the same with an N at base 15, 16, 31, 32, 33 or L - 1 of half the
    reads (every tile has some); long: ONE tile that fits a wavefront's stage and fills its lists — sixteen reads of 470 to 1000
    bases among reads of 150; long_equal: one tile of reads of 480 bases (must_restart holds for both, k <= 64).  In long_equal_n a
    read WITH an N need not overflow its list by itself (its clean windows may be fewer than twelve runs' worth): the restart rests
    on the tile's reads without one — read 0 never gets an N."""
    out = []
    if kind == "long":
        ll = [int(rng.integers(470, 1001)) if n % 4 == 1 else 150 for n in range(64)]
        return [bytes(_read(rng, gs, L)) for L in ll]
    if kind.startswith("long_equal"):
        ls, tile = [480], 64
    ls = lengths(k) if ls is None else ls
    per_tile = [[L] * tile for L in ls] if "equal" in kind else [list(rng.choice(ls, size=tile)) for _ in range(4)]
    for t in per_tile:
        for n, L in enumerate(t):
            r = _read(rng, gs, int(L))
            if kind.endswith("_n") and n % 64 != 0 and (n % 64 == 7 or rng.random() < 0.5):
                at = [p for p in (15, 16, 31, 32, 33, int(L) - 1) if p < L]
                r[at[int(rng.integers(0, len(at)))]] = ord("N")
            out.append(bytes(r))
    return out


def flat(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offs
