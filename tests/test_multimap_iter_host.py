"""--multimap_iterations on the host: the definition (metalign_amd/multimap.py) against the hand example and today's one step, the
library's host routine (mg_multimapped_shares_iter) against the definition bit for bit, the stop rule, the flags and their refusals,
and the arithmetic of mg_multimap_core.h compiled with g++ (plain, and with the address and undefined-behaviour sanitizers)."""
import argparse
import copy
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import multimap_cases as mc
from metalign_amd import _hip, cli
from metalign_amd import map_and_profile as mp
from metalign_amd import multimap as mmdef

HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    """Bit for bit, NaN included."""
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def test_hand_example_and_conservation():
    for n, want in ((1, mc.HAND_AFTER_1), (2, mc.HAND_AFTER_2)):
        extra, touched, ran, _ = mmdef.iterate(mc.HAND_W0, mc.HAND_OFF, mc.HAND_TAX, mc.HAND_HITLEN, None, n, 0.0)
        w = [a + b for a, b in zip(mc.HAND_W0, extra)]
        assert ran == n and all(touched)
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(w, want)), (n, w)
        assert abs(sum(w) - 900.0) <= 1e-12 * 900.0
    assert [round(x, 6) for x in mc.HAND_AFTER_2] == [428.571429, 282.539683, 188.888889]
    t2a = {"A": [5, 300.0], "B": [5, 100.0], "C": [5, 100.0]}
    assert mmdef.resolve(t2a, ["A", "B", "C", "D"], mc.HAND_OFF, mc.HAND_TAX, mc.HAND_HITLEN, None, 2, 0.0)[0] == 2
    assert all(abs(t2a[k][1] - b) <= 1e-12 * b for k, b in zip("ABC", mc.HAND_AFTER_2))
    for bad in (dict(max_iter=0), dict(tol=-1.0), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            mmdef.iterate(mc.HAND_W0, mc.HAND_OFF, mc.HAND_TAX, mc.HAND_HITLEN, **bad)


@pytest.mark.parametrize("trial", range(4))
def test_one_iteration_of_the_definition_is_todays_step_bit_for_bit(trial):
    rng = np.random.default_rng(100 + trial)
    T = int(rng.integers(3, 60))
    off, tax, hitlen, w0, glen = mc.random_csr(rng, T, int(rng.integers(1, 3000)), fractional=trial % 2 == 1)
    taxids = ["t%d" % i for i in range(T)]
    t2i = {t: [float(glen[i]), "strain", "x|y"] for i, t in enumerate(taxids)}
    t2a = {t: [3, float(w0[i])] + t2i[t] for i, t in enumerate(taxids) if w0[i] == w0[i]}
    mm = dict(taxids=taxids, mm_offsets=off, mm_tax=tax, mm_hitlen=hitlen)
    for ln in (False, True):
        want = mp.resolve_multi_prop_csr(argparse.Namespace(verbose=False, length_normalize=ln), copy.deepcopy(t2a), mm, t2i)
        got = copy.deepcopy(t2a)
        assert mmdef.resolve(got, taxids, off, tax, hitlen, glen if ln else None, 1, 0.0)[0] == 1
        assert got == want and any(got[k][1] != t2a[k][1] for k in got)


_RANDOM = [(seed, None, None) for seed in range(5)] + [(77, 700, 40_000)]


@pytest.mark.parametrize("seed,T,nreads", _RANDOM)
def test_library_routine_equals_the_definition_bit_for_bit(seed, T, nreads):
    """Repeated taxa, NaN taxa, empty reads, zero and fractional weights, genome lengths; N in 1, 2, 5; the serial loop and the
    threaded one; extra, touched, iterations_run and last_change."""
    rng = np.random.default_rng(seed)
    T = T or int(rng.integers(3, 60))
    nreads = nreads if nreads is not None else int(rng.integers(0, 4000))
    off, tax, hitlen, w0, glen = mc.random_csr(rng, T, nreads, fractional=seed % 2 == 1)
    for gl in (None, glen):
        for n in (1, 2, 5):
            want = mc.definition(w0, off, tax, hitlen, gl, n, 0.0)
            assert want[2] == n
            for threads in (1, 2, 8):
                _hip.debug_set("shares_threads", threads)
                try:
                    got = _hip.multimapped_shares_iter(off, tax, hitlen, w0, gl, n, 0.0)
                finally:
                    _hip.debug_set("shares_threads", 0)
                assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, n, threads)
                assert got[2] == want[2] and _same([got[3]], [want[3]])
    if nreads:  # the iteration does move the weights
        a, b = mc.definition(w0, off, tax, hitlen, None, 1)[0], mc.definition(w0, off, tax, hitlen, None, 5)[0]
        assert not _same(a, b)
    # max_iter = 1 is the one-step routine
    one = _hip.multimapped_shares(off, tax, hitlen, w0, glen)
    it = _hip.multimapped_shares_iter(off, tax, hitlen, w0, glen, 1, 0.0)
    assert _same(one[0], it[0]) and np.array_equal(one[1], it[1])


def test_stop_rule():
    rng = np.random.default_rng(4)
    off, tax, hitlen, w0, glen = mc.random_csr(rng, 25, 3000)
    changes = []
    assert mc.definition(w0, off, tax, hitlen, None, 12, 0.0, changes)[2] == 12 and len(changes) == 12
    assert all(a > b > 0 for a, b in zip(changes, changes[1:7])), changes
    tol = math.sqrt(changes[2] * changes[3])
    assert changes[3] < tol < changes[2]
    for fn in (mc.definition, lambda w, o, t, h, *rest: _hip.multimapped_shares_iter(o, t, h, w, *rest)):
        got = fn(w0, off, tax, hitlen, None, 12, tol)
        assert got[2] == 4 and got[3] == changes[3]
        assert _same(got[0], mc.definition(w0, off, tax, hitlen, None, 4, 0.0)[0])
        assert fn(w0, off, tax, hitlen, None, 12, 0.0)[2] == 12
        assert fn(w0, off, tax, hitlen, None, 3, tol)[2] == 3  # max_iter first
    for bad in ((0, 0.0), (1, -1e-9), (1, float("nan"))):
        with pytest.raises(_hip.HipError):
            _hip.multimapped_shares_iter(off, tax, hitlen, w0, None, *bad)


def test_a_read_whose_weights_are_all_zero_is_decided_anew_with_every_weights():
    off, tax, hl, w0 = mc.ZERO_OFF, mc.ZERO_TAX, mc.ZERO_HITLEN, mc.ZERO_W0
    w = [None if x != x else x for x in w0]
    # one step with the starting weights: reads 0 and 3 (only taxon 0, weight 0.0) are skipped; read 2 gives taxon 0 a share of 0.0
    extra, touched = mmdef.step(w, off, tax, hl)
    assert extra == [0.0, 100 * 50 / 200 + 60.0, 100 * 150 / 200, 0.0] and touched == [True, True, True, False]
    # the same reads with a weight that has grown: both take part, whole
    extra2, _ = mmdef.step([5.0] + w[1:], off, tax, hl)
    assert extra2[0] == 80.0 + 40.0 + 60 * 5.0 / 55.0
    # inside one run a weight of exactly 0.0 cannot grow: the reads stay out of every iteration, host routine and definition alike
    for n in (1, 2, 6):
        want = mc.definition(w0, off, tax, hl, None, n)
        got = _hip.multimapped_shares_iter(off, tax, hl, w0, None, n, 0.0)
        assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0][0] == 0.0
        assert abs(float(np.nansum(mc.weights(w0, got[0]))) - (200.0 + 160.0)) < 1e-9  # reads 1 and 2 hand out their 160 bases


def test_the_flags_exist_on_both_tools():
    for tool in ("map_and_profile", "metalign"):
        acts = {a.dest: a for a in cli.parser_for(tool)._actions}
        n, tol = acts["multimap_iterations"], acts["multimap_tol"]
        assert n.default == 1 and n.type is int and n.option_strings == ["--multimap_iterations"]
        assert tol.default == 1e-8 and tol.type is float and tol.option_strings == ["--multimap_tol"]


@pytest.mark.parametrize("over,word", [({"multimap_iterations": 0}, "--multimap_iterations"), ({"multimap_iterations": -3}, "--multimap_iterations"),
                                       ({"multimap_tol": -1e-9}, "--multimap_tol"),
                                       ({"multimap_iterations": 2, "low_mem": True}, "--low_mem")])
def test_refusals_fire_before_any_input_is_opened(monkeypatch, tmp_path, over, word):
    import stage_c_checks as sc
    from metalign_amd import metalign, select_db

    def never(*a, **k):
        raise AssertionError("refused before the GPU, the library or an input is touched")
    monkeypatch.setattr(_hip.Hip, "get", never)
    monkeypatch.setattr(_hip, "load_library", never)
    monkeypatch.setattr(select_db, "dist_context", never)
    monkeypatch.setattr(select_db, "select_main", never)
    monkeypatch.setattr(mp, "get_acc2info", never)
    out = tmp_path / "o.cami"
    args = sc.make_args(str(tmp_path / "missing.sam"), str(tmp_path / "missing_db_info.txt"), str(out), over)
    with pytest.raises(SystemExit) as e:
        mp.map_main(args)
    assert word in str(e.value.code) and str(e.value.code).startswith("Error: ") and not out.exists()
    argv = [str(tmp_path / "missing.fq"), str(tmp_path / "data")]
    for k, v in over.items():
        argv += ["--" + k] if v is True else ["--%s=%s" % (k, v)]
    with pytest.raises(SystemExit) as e:
        metalign.main(argv)
    assert word in str(e.value.code) and not (tmp_path / "data").exists()
    # what is allowed passes the check
    mp.check_multimap_flags(argparse.Namespace(multimap_iterations=1, multimap_tol=0.0, low_mem=True))
    mp.check_multimap_flags(argparse.Namespace(multimap_iterations=30, multimap_tol=1e-8, low_mem=False))
    mp.check_multimap_flags(argparse.Namespace(low_mem=True))  # (a caller's Namespace without the flags: one step)


# ---- mg_multimap_core.h on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("multimap") / ("host_multimap_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-Wall"] + flags + ["-o", out, os.path.join(HERE, "host_multimap_check.cpp")])
    return out


def test_core_header_arithmetic_equals_the_definition(exe, tmp_path):
    rng = np.random.default_rng(12)
    off, tax, hitlen, w0, glen = mc.random_csr(rng, 40, 2500, fractional=True)
    w = [None if x != x else float(x) for x in w0]
    ints = lambda a: [int(x) for x in a]  # noqa: E731
    extra1, touched1 = mmdef.step(w, ints(off), ints(tax), ints(hitlen))
    w1 = mmdef.new_weights(w, extra1, touched1)
    extra2, touched2 = mmdef.step(w1, ints(off), ints(tax), ints(hitlen))
    w2 = mmdef.new_weights(w, extra2, touched2)
    nan = float("nan")
    blob = struct.pack("<I", len(w))
    for t in range(len(w)):
        blob += struct.pack("<ddd", nan if w[t] is None else w[t], nan if w1[t] is None else w1[t], extra2[t])
    shares = [(3.0, 7.0, 100.0, 0.0), (1 / 3, 0.7, 151.0, 4321.0), (0.0, 5.0, 30.0, 0.0), (5.0, 5.0, 2.0 ** 40, 1234.5)]
    blob += struct.pack("<I", len(shares)) + b"".join(struct.pack("<dddd", *s) for s in shares)
    stops = [(1, 1, 0.0, 1.0), (1, 2, 0.0, 0.0), (2, 5, 1e-8, 1e-8), (2, 5, 1e-8, 1.0000001e-8), (5, 5, 1e-8, 1.0), (3, 9, 0.0, 0.0)]
    blob += struct.pack("<I", len(stops)) + b"".join(struct.pack("<IIdd", *s) for s in stops)
    lists = [[0], [1], [0, 1], [1, 2], [0, 1, 2], list(range(300)), list(range(1, 301)), [2 ** 32 - 1], []]
    blob += struct.pack("<I", len(lists)) + b"".join(struct.pack("<I%dI" % len(x), len(x), *x) for x in lists)
    p = tmp_path / "in.bin"
    p.write_bytes(blob)
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    rows = [ln.split() for ln in out.stdout.decode().splitlines()]
    got_w = [float.fromhex(r[1]) for r in rows if r[0] == "W"]
    assert _same(got_w, [nan if x is None else x for x in w2])
    assert [float.fromhex(r[1]) for r in rows if r[0] == "C"] == [mmdef.change(w2, w1)]
    want_p = [(a / b) * h / g if g else (a / b) * h for a, b, h, g in shares]
    assert [float.fromhex(r[1]) for r in rows if r[0] == "P"] == want_p
    assert [int(r[1]) for r in rows if r[0] == "S"] == [1, 0, 1, 0, 1, 0]
    hashes = [int(r[1]) for r in rows if r[0] == "H"]
    assert len(set(hashes)) == len(lists) and all(h != 2 ** 64 - 1 for h in hashes)
