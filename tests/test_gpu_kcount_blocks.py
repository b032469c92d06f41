"""k_count_kmers on the tiles that the walk in blocks of 32 candidates can go wrong at (kcount_blocks_cases.py: read lengths
around every block and dword boundary, equal and ragged, a base that is no base at those boundaries, and tiles that fit the
stage yet hold reads with more runs than a list has slots — ragged, equal-length, equal-length with an N: the walk of the usual
tile starts anew off a multiple of 16 in all three modes), k = 50, 51, 53 (the new
walk) and 60 (the general one), exact counts and saturating ones, against the oracle's mgo_refpipe_count_kmers.  Bit-exact."""
import numpy as np
import pytest

from kcount_blocks_cases import GLEN, KINDS, NGEN, flat, genomes, lengths, must_restart, reads

pytestmark = pytest.mark.gpu

KS = (50, 51, 53, 60)
_tables = {}


def _table(hip, oracle_lib, k):
    """the sketched k-mers of 6 genomes x 3 kb, indexed: built once per k"""
    if k not in _tables:
        rng = np.random.default_rng(7100 + k)
        gs = genomes(rng)
        gb, go = np.concatenate(gs), (np.arange(NGEN + 1) * GLEN).astype(np.uint64)
        h, khi, klo, o = hip.sketch_genomes_kmers(gb, go, k, 200)
        table = hip.refdb_build(h, khi, klo, o, [k])
        table.index_kmers()
        _tables[k] = (gs, table, oracle_lib.refpipe_build(h, khi, klo, o, [k]))
    return _tables[k]


# (the ten equal-length tiles in two cases of five, every other length each: 320 reads a case)
PARAMS = [(k, kind, half) for k in KS for kind in KINDS for half in ((0, 1) if kind.startswith("equal") else (0,))]


@pytest.mark.parametrize("k,kind,half", PARAMS, ids=["-".join(map(str, p)) for p in PARAMS])
def test_counts_match_the_oracle(hip, oracle_lib, k, kind, half):
    gs, table, want_table = _table(hip, oracle_lib, k)
    rng = np.random.default_rng(7200 + 10 * k + len(kind) + half)
    rd = reads(rng, gs, k, kind, ls=lengths(k)[half::2] if kind.startswith("equal") else None)  # 64 to 320 reads
    if kind.startswith("long"):  # more windows than twelve runs can cover, in a tile that fits the stage: the usual tile's walk restarts
        assert len(rd) == 64 and must_restart(k, rd)
    rb, ro = flat(rd)
    d_b, d_o = hip.array(np.concatenate([rb, np.zeros(64, np.uint8)])), hip.array(ro)
    try:
        for cs in (0, 3):
            hip.count_saturation(cs)
            want, seen = oracle_lib.refpipe_count_kmers(rb, ro, k, want_table["kmer_hi"], want_table["kmer_lo"], cs=cs)
            kc = table.kmer_counts()
            kc.add_dev(d_b.ptr, d_o.ptr, len(rd), int(ro[-1]))
            hip.sync()
            got, st = kc.download(), kc.stats()
            kc.free()
            assert np.array_equal(got, want), (cs, np.flatnonzero(got != want)[:10])
            assert st["kmers"] == seen
            assert want.sum() > 0
    finally:
        hip.count_saturation(3)
        d_b.free()
        d_o.free()
