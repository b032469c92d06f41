"""CPU: build_db._splice — the entries of host-parsed genomes put back into a device batch's arrays — against a per-genome
restatement, on random batches (empty genomes, several undecided ones, the first and the last among them)."""
import numpy as np

from metalign_amd import build_db


def test_splice_equals_the_per_genome_restatement():
    rng = np.random.default_rng(0)
    for _ in range(300):
        g = int(rng.integers(1, 9))
        lens = rng.integers(0, 5, g)
        o = np.zeros(g + 1, np.uint64)
        o[1:] = np.cumsum(lens)
        arrays = (np.arange(int(o[-1]), dtype=np.uint64), 3 * np.arange(int(o[-1]), dtype=np.uint64))
        und = sorted(rng.choice(g, size=int(rng.integers(1, g + 1)), replace=False).tolist())
        hlens = rng.integers(0, 5, len(und))
        ho = np.zeros(len(und) + 1, np.uint64)
        ho[1:] = np.cumsum(hlens)
        harrays = (1000 + np.arange(int(ho[-1]), dtype=np.uint64), 7000 + np.arange(int(ho[-1]), dtype=np.uint64))
        out, oo = build_db._splice(arrays, o, und, harrays, ho)
        assert oo.dtype == np.uint64 and all(a.dtype == np.uint64 for a in out)
        assert list(np.diff(oo.astype(np.int64))) == [int(hlens[und.index(f)]) if f in und else int(lens[f]) for f in range(g)]
        for c in range(2):
            want = []
            for f in range(g):
                if f in und:
                    j = und.index(f)
                    want += list(harrays[c][int(ho[j]):int(ho[j + 1])])
                else:
                    want += list(arrays[c][int(o[f]):int(o[f + 1])])
            assert list(out[c]) == want
