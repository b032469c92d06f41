"""The walk in blocks of 32 candidates (mg_kcount_core.h: kc_walk32, k with 32 or 33 candidates) and the general walk beside it
(k = 49, 52, 60), compiled for the host, against the oracle's mgo_refpipe_count_kmers: tiles whose reads end around every
block and dword boundary, equal and ragged, with and without a base that is no base at those boundaries, and reads of 470 to
1000 bases (among reads of 150, or 64 of 480: all three modes) with lists of three and twelve slots — the walk then starts anew at windows that are no multiple of 16 (rounded
down, the windows before masked).  Counts and the reads' total of k-mers are compared exactly."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from kcount_blocks_cases import GLEN, KINDS, NGEN, flat, genomes, must_restart, reads
from test_kcount_core_host import pack_table, unpack

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (49, 50, 51, 52, 53, 60, 63)  # both walks and both joining points (W = 31 | 32, 33 | 34), the stock preset's k = 60


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kcblocks") / "host_kcount_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-o", exe, os.path.join(HERE, "host_kcount_check.cpp")])
    return exe


# lists of three slots: the long reads (MODE 2), and for k = 50, 51 (W = 32, 33) the equal-length tiles with and without an N as
# well — MODE 1, whose restarted calls run the tail block's code for every block, and MODE 0
def _caps(k, kind):
    return (3, 12) if kind == "long" or (k in (50, 51) and kind in ("equal", "equal_n")) else (12,)


PARAMS = [(k, kind, cap, lead) for k in KS for kind in KINDS for cap in _caps(k, kind) for lead in (0, 5)]


@pytest.mark.parametrize("k,kind,cap,lead", PARAMS, ids=["-".join(map(str, p)) for p in PARAMS])
def test_counts_equal_the_oracle(checker, k, kind, cap, lead):
    oracle.build()
    rng = np.random.default_rng(7000 + 10 * k + lead)
    gs = genomes(rng)
    gb, go = np.concatenate(gs), (np.arange(NGEN + 1) * GLEN).astype(np.uint64)
    _, khi, klo, _ = oracle.sketch_genomes_kmers(gb, go, k, 200)
    table = [unpack(a, b, k) for a, b in zip(khi, klo)]
    rd = reads(rng, gs, k, kind)
    text = ("%d %d %d %d %d %d %d\n" % (k, cap, len(table), len(rd), lead, 0, 0)).encode() + b"".join(t + b"\n" for t in table) + \
        b"".join(r + b"\n" for r in rd)
    out = subprocess.run([checker], input=text, capture_output=True, check=True).stdout.decode().split("\n")
    got = np.array([int(x) for x in out[:len(table)]], dtype=np.uint32)
    tail = out[len(table)].split()
    bases, offs = flat(rd)
    khi, klo = pack_table(table, k)
    want, seen = oracle.refpipe_count_kmers(bases, offs, k, khi, klo, cs=0)
    assert int(tail[1]) == seen, "k-mers of the reads"
    assert np.array_equal(got, want), "counts differ at %s" % np.flatnonzero(got != want)[:10]
    assert want.sum() > 0
    if kind.startswith("long"):
        assert must_restart(k, rd[:64], cap)
    if kind.startswith("long") or cap == 3:
        assert int(tail[7]) > 0, "these reads must have filled a list"
