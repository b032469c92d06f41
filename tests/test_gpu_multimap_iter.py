"""-m gpu: --multimap_iterations on the device — mg_profile_mm_iterate_dev (mg_multimap.hip: the classes of reads with the same taxa,
an iteration over classes) and the command line.  The expectation is always metalign_amd/multimap.py, or the library's host routine,
which tests/test_multimap_iter_host.py ties to it bit for bit."""
import ctypes
import math
import random

import numpy as np
import pytest

import bamgen
import multimap_cases as mc
import samgen
import stage_c_checks as sc
from metalign_amd import _hip
from metalign_amd import map_and_profile as mp
from metalign_amd import multimap as mmdef

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 8
SENTINEL = -12345.678


def _iterate(hip, resident, w0, glen, n, tol=0.0):
    """mg_profile_mm_iterate_dev into a buffer with guard words on both sides -> (extra, iterations_run, last_change, nclasses)."""
    T = len(w0)
    d_w = hip.array(np.ascontiguousarray(w0, dtype=np.float64))
    d_l = hip.array(np.ascontiguousarray(glen, dtype=np.float64)) if glen is not None else None
    d_x = hip.array(np.full(T + 2 * GUARD, SENTINEL, dtype=np.float64))
    ran, change, ncls = ctypes.c_uint32(0), ctypes.c_double(-1.0), ctypes.c_uint64(2 ** 40)
    try:
        hip._chk(hip.lib.mg_profile_mm_iterate_dev(resident.shard.handle, _hip._vp(d_w.ptr), _hip._vp(d_l.ptr if d_l else None),
                                                   ctypes.c_uint32(n), ctypes.c_double(tol), _hip._vp(d_x.ptr + 8 * GUARD),
                                                   ctypes.byref(ran), ctypes.byref(change), ctypes.byref(ncls)))
        x = d_x.download()
    finally:
        d_w.free()
        d_x.free()
        if d_l:
            d_l.free()
    assert np.all(x[:GUARD] == SENTINEL) and np.all(x[T + GUARD:] == SENTINEL), "guard words around d_extra"
    return x[GUARD:T + GUARD].copy(), int(ran.value), float(change.value), int(ncls.value)


def _classes(off, tax, w0):
    return len({tuple(sorted({t for t in row if w0[t] == w0[t]})) for row in mc.as_lists(off, tax)} - {()})


def _rel(a, b):
    """Largest relative deviation of the weights a from the weights b over the taxa with an entry."""
    ok = ~np.isnan(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    if not ok.any():
        return 0.0
    d = np.abs(a[ok] - b[ok])
    return float(np.max(np.where(b[ok] != 0, d / np.where(b[ok] != 0, b[ok], 1.0), d)))


# ---- random shapes -------------------------------------------------------------------------------------------------------------
class Shape:
    pass


def _random_shape(hip, ntax, seed):
    """60 000 records, about 45 % of them opening a read (as test_device_multimap_equals_host_resolution); some taxa dropped."""
    rng = np.random.default_rng(seed)
    nrec, nref = 60000, 400 if ntax < 400 else 3 * ntax
    recs = np.zeros(nrec, dtype=_hip.REC_DTYPE)
    new = rng.random(nrec) < 0.45
    new[0] = True
    recs["ref_new"] = rng.integers(0, nref, size=nrec).astype(np.uint32) | (new.astype(np.uint32) << 31)
    recs["total"] = 100
    recs["matched"] = rng.integers(30, 101, size=nrec)
    recs["flag_len"] = rng.choice([0, 16, 256, 272], size=nrec).astype(np.uint32) | (np.uint32(100) << 12)
    ref2tax = rng.integers(0, ntax, size=nref).astype(np.uint32)
    s = Shape()
    host = hip.profile_assign(recs, ref2tax, ntax, 0.5)
    s.dev = hip.profile_assign_resident(recs, ref2tax, ntax, 0.5)
    s.off, s.tax, s.hitlen = host["mm_offsets"], host["mm_tax"], host["mm_hitlen"]
    assert 3000 < s.dev["mm_nreads"] == len(s.hitlen) <= 20000  # (few enough for the decimal yardstick: no cut needed)
    s.w0 = np.where((host["count"] > 0) & (np.arange(ntax) % 5 != 0), host["bases"].astype(np.float64), np.nan)
    s.glen = 1000.0 + 13.0 * np.arange(ntax)
    s.rng = rng
    return s


ITERS = (1, 2, 7)
ALL_ITERS = (1, 2, 4, 7)  # (4: where the stop-rule test ends)


@pytest.fixture(scope="module")
def shape37(hip):
    """ntax = 37 (the LDS accumulation).  Yardstick: the definition in decimal at 50 digits.  d_ref: the largest relative deviation from
    it of the float64 definition over the given read order and 5 seeded permutations of the reads."""
    s = _random_shape(hip, 37, 5)
    s.yard, s.d_ref = {}, {}
    for norm in (False, True):
        gl = s.glen if norm else None
        yard = mc.decimal_weights(s.w0, s.off, s.tax, s.hitlen, gl, ALL_ITERS)
        orders = [(s.off, s.tax, s.hitlen)] + [mc.permuted(np.random.default_rng(900 + k), s.off, s.tax, s.hitlen) for k in range(5)]
        floats = [mc.trajectory(s.w0, o, t, h, gl, ALL_ITERS) for o, t, h in orders]
        for n in ALL_ITERS:
            s.yard[norm, n] = yard[n]
            s.d_ref[norm, n] = max(mc.rel_dev(f[n], yard[n]) for f in floats)
    yield s
    s.dev["resident"].free()


@pytest.fixture(scope="module")
def shape2049(hip):
    """ntax = 2049 (global atomics).  The spread of the host routine over 5 seeded permutations of the reads, host against host."""
    s = _random_shape(hip, 2049, 6)
    s.host, s.spread = {}, {}
    perms = [mc.permuted(np.random.default_rng(700 + k), s.off, s.tax, s.hitlen) for k in range(5)]
    for norm in (False, True):
        gl = s.glen if norm else None
        for n in ITERS:
            base = mc.weights(s.w0, _hip.multimapped_shares_iter(s.off, s.tax, s.hitlen, s.w0, gl, n, 0.0)[0])
            s.host[norm, n] = base
            s.spread[norm, n] = max(_rel(mc.weights(s.w0, _hip.multimapped_shares_iter(o, t, h, s.w0, gl, n, 0.0)[0]), base)
                                    for o, t, h in perms)
    yield s
    s.dev["resident"].free()


@pytest.mark.parametrize("n", ITERS)
@pytest.mark.parametrize("norm", [False, True])
def test_device_within_eight_d_ref_of_the_decimal_yardstick(hip, shape37, norm, n):
    """Measured on the MI355X: without genome lengths d_ref 2.1e-15 .. 2.4e-15 and the device 2.2e-16 .. 3.8e-16 from
    the yardstick; with them (the additions are small beside w0) d_ref 6.6e-17 .. 1.1e-16, the device 6.5e-17 .. 9.4e-17."""
    s = shape37
    extra, ran, change, ncls = _iterate(hip, s.dev["resident"], s.w0, s.glen if norm else None, n)
    dev = mc.rel_dev(mc.weights(s.w0, extra), s.yard[norm, n])
    print("ntax 37 norm %d N %d: d_ref %.3g device %.3g classes %d of %d reads" % (norm, n, s.d_ref[norm, n], dev, ncls, len(s.hitlen)))
    assert ran == n and ncls == _classes(s.off, s.tax, s.w0) < len(s.hitlen)
    assert s.d_ref[norm, n] > 0 and dev <= 8 * s.d_ref[norm, n]
    want_change = []
    mc.definition(s.w0, s.off, s.tax, s.hitlen, s.glen if norm else None, n, 0.0, want_change)
    assert abs(change - want_change[-1]) <= 16 * s.d_ref[norm, n]  # (a difference of two weights, each within 8 d_ref)
    assert np.array_equal(np.isnan(s.w0), np.isnan(mc.weights(s.w0, extra)))


@pytest.mark.parametrize("n", ITERS)
@pytest.mark.parametrize("norm", [False, True])
def test_device_within_eight_spreads_of_the_host_above_the_lds_limit(hip, shape2049, norm, n):
    """Measured on the MI355X: spread 6.0e-16 .. 7.4e-16 and device against host 4.4e-16 .. 6.8e-16 without genome
    lengths; 1.4e-16 and 0 .. 1.4e-16 with them."""
    s = shape2049
    extra, ran, _, ncls = _iterate(hip, s.dev["resident"], s.w0, s.glen if norm else None, n)
    dev = _rel(mc.weights(s.w0, extra), s.host[norm, n])
    print("ntax 2049 norm %d N %d: spread %.3g device %.3g classes %d of %d reads" % (norm, n, s.spread[norm, n], dev, ncls, len(s.hitlen)))
    assert ran == n and ncls == _classes(s.off, s.tax, s.w0)
    assert s.spread[norm, n] > 0 and dev <= 8 * s.spread[norm, n]


def test_one_iteration_against_the_one_step_kernel(hip, shape37, shape2049):
    """max_iter = 1 through the new entry point against mg_profile_resolve_multimapped_dev on the same shard: two orders of the same
    one step.  The weights w0 + extra of the two kernels lie within the tolerance of the other device tests of each other: 8 d_ref of
    the decimal yardstick at ntax = 37, 8 permutation spreads of the host routine at ntax = 2049 (both for one iteration)."""
    for s, tolerance in ((shape37, shape37.d_ref), (shape2049, shape2049.spread)):
        for norm in (False, True):
            gl = s.glen if norm else None
            old = s.dev["resident"].resolve_multimapped(s.w0, gl)
            new = _iterate(hip, s.dev["resident"], s.w0, gl, 1)[0]
            bound = 8 * tolerance[norm, 1]
            apart = _rel(mc.weights(s.w0, new), mc.weights(s.w0, old))
            print("ntax %d norm %d: bound %.3g, one-step kernel and class form %.3g apart" % (len(s.w0), norm, bound, apart))
            assert np.array_equal(old == 0, new == 0) and np.any(old != 0)
            assert bound > 0 and apart <= bound
            # and the wrappers of both profile classes
            got = s.dev["resident"].iterate_multimapped(s.w0, gl, 1, 0.0)
            assert got[1] == 1 and got[3] == _classes(s.off, s.tax, s.w0)
            assert _rel(mc.weights(s.w0, got[0]), mc.weights(s.w0, new)) <= bound


def test_stop_rule_on_the_device(hip, shape37):
    s = shape37
    c = []
    mc.definition(s.w0, s.off, s.tax, s.hitlen, None, 6, 0.0, c)
    assert c[2] > c[3] > 0
    tol = math.sqrt(c[2] * c[3])  # (a factor of about 1.5 from either: far above rounding)
    extra, ran, change, _ = _iterate(hip, s.dev["resident"], s.w0, None, 12, tol)
    assert ran == 4 and abs(change - c[3]) <= 16 * s.d_ref[False, 4]
    assert mc.rel_dev(mc.weights(s.w0, extra), s.yard[False, 4]) <= 8 * s.d_ref[False, 4]
    assert _iterate(hip, s.dev["resident"], s.w0, None, 12, 0.0)[1] == 12
    assert _iterate(hip, s.dev["resident"], s.w0, None, 3, tol)[1] == 3
    for bad in ((0, 0.0), (1, -1e-9), (1, float("nan"))):
        with pytest.raises(_hip.HipError) as e:
            _iterate(hip, s.dev["resident"], s.w0, None, *bad)
        assert e.value.code == _hip.ERR_ARG


def test_a_hash_collision_splits_a_class_and_never_merges_two(hip, shape37, knobs):
    s = shape37
    plain = _iterate(hip, s.dev["resident"], s.w0, None, 7)
    knobs("mm_hash_bits", 2)  # four hash values for hundreds of different lists: every run of equal hashes holds many lists
    split = _iterate(hip, s.dev["resident"], s.w0, None, 7)
    knobs("mm_hash_bits", 0)
    assert split[3] > plain[3] == _classes(s.off, s.tax, s.w0)
    for got in (plain, split):
        assert mc.rel_dev(mc.weights(s.w0, got[0]), s.yard[False, 7]) <= 8 * s.d_ref[False, 7]


# ---- edge shapes ---------------------------------------------------------------------------------------------------------------
T_EDGE = 320
DROPPED = (5, 6, 100, 317)


def _edge_w0(T=T_EDGE):
    w = np.array([10.0 + (t * 37) % 101 + 0.25 * (t % 3) for t in range(T)])
    w[list(d for d in DROPPED if d < T)] = np.nan
    return w


def _random_lists(seed, n):
    rng = random.Random(seed)
    return [[rng.choice([1, 2, 3, 4, 5, 7, 8, 9]) for _ in range(rng.randrange(2, 6))] for _ in range(n)]


_LONG = list(range(10, 310))
_EDGES = {
    # name: (lists, classes expected or None = count them)
    "no_multimapped_read": ([], 0),
    "every_taxon_dropped": ([[5, 6], [6, 5], [5, 5, 6], [100, 317]], 0),
    "one_read": ([[1, 2, 3]], 1),
    "reads_63": (_random_lists(63, 63), None),
    "reads_64": (_random_lists(64, 64), None),
    "reads_65": (_random_lists(65, 65), None),
    "reads_257": (_random_lists(257, 257), None),
    "length_1_after_dropping": ([[1, 5], [6, 2], [5, 3, 6], [1, 100]], 3),
    "length_2": ([[1, 2], [2, 1], [3, 4]], 2),
    "length_300": ([random.Random(1).sample(_LONG, 300), random.Random(2).sample(_LONG, 300), _LONG[:299] + [9], [1, 2]], 3),
    "forty_copies_of_one_taxon": ([[7] * 40, [7, 8], [8] * 40 + [7]], 2),
    "all_reads_in_one_class": ([random.Random(k).sample([1, 2, 3], 3) + [random.Random(k).choice([1, 2, 3, 5])] for k in range(200)], 1),
    "every_read_a_class_of_its_own": ([[t, t + 1] for t in range(110, 310)], 200),
    "one_set_in_different_orders": ([[1, 2, 3], [3, 2, 1], [2, 3, 1, 1], [2, 5, 1, 3], [6, 3, 3, 2, 1, 100]], 1),
}


@pytest.mark.parametrize("name", list(_EDGES))
def test_edge_shapes(hip, name):
    """Against the definition.  Bound: one iteration's additions carry (n + m + 3) u relative in any order (n taxa in the longest
    list, m reads: see test_one_iteration_against_the_one_step_kernel), and a relative error e in the weights becomes at most 2 e in
    the next shares (w / den: once through w, once through den) -> after N iterations (2^N - 1) (n + m + 3) u, counted from both sides."""
    lists, want_classes = _EDGES[name]
    hitlens = [30 + (7 * k) % 121 for k in range(len(lists))]
    recs = mc.records(_hip.REC_DTYPE, lists, hitlens)
    r2t = np.arange(T_EDGE, dtype=np.uint32)
    host = hip.profile_assign(recs, r2t, T_EDGE, 0.5)
    off, tax = mc.csr(lists)
    assert np.array_equal(host["mm_offsets"], off) and np.array_equal(host["mm_tax"], tax)  # the CSR is the intended one
    assert np.array_equal(host["mm_hitlen"], np.array(hitlens, dtype=np.uint64))
    dev = hip.profile_assign_resident(recs, r2t, T_EDGE, 0.5)
    w0 = _edge_w0()
    try:
        assert dev["mm_nreads"] == len(lists)
        for gl in (None, 1000.0 + 13.0 * np.arange(T_EDGE)):
            for n in (1, 3):
                extra, ran, change, ncls = _iterate(hip, dev["resident"], w0, gl, n)
                want = mc.definition(w0, off, tax, hitlens, gl, n, 0.0)
                assert ran == n == want[2]
                assert ncls == (want_classes if want_classes is not None else _classes(off, tax, w0))
                bound = 2 * (2 ** n - 1) * (max([len(x) for x in lists] + [0]) + len(lists) + 3) * U
                assert np.array_equal(extra != 0, want[0] != 0)
                assert np.all(np.abs(extra - want[0]) <= bound * np.abs(want[0])), name
                assert abs(change - want[3]) <= 2 * bound  # (a difference of two weights, each within the bound)
        if want_classes == 0:  # nothing to share: one iteration when a tolerance asks, else all of them
            assert _iterate(hip, dev["resident"], w0, None, 5, 1e-8)[1] == 1
    finally:
        dev["resident"].free()


def test_reads_whose_weights_are_all_zero_stay_out(hip):
    """The weight-0 case of the CPU tests: reads 0 and 3 (their only kept taxon weighs 0.0) are skipped in every iteration, read 2 gives
    taxon 0 a share of exactly 0.0."""
    lists, hitlens = mc.as_lists(mc.ZERO_OFF, mc.ZERO_TAX), mc.ZERO_HITLEN
    recs = mc.records(_hip.REC_DTYPE, lists, hitlens)
    host = hip.profile_assign(recs, np.arange(4, dtype=np.uint32), 4, 0.5)
    assert np.array_equal(host["mm_offsets"], np.array(mc.ZERO_OFF, dtype=np.uint64)) and list(host["mm_tax"]) == mc.ZERO_TAX
    dev = hip.profile_assign_resident(recs, np.arange(4, dtype=np.uint32), 4, 0.5)
    w0 = np.array(mc.ZERO_W0)
    try:
        for n in (1, 2, 6):
            extra, ran, _, ncls = _iterate(hip, dev["resident"], w0, None, n)
            want = mc.definition(w0, mc.ZERO_OFF, mc.ZERO_TAX, hitlens, None, n)[0]
            assert ran == n and ncls == 3 and extra[0] == 0.0 and extra[3] == 0.0
            assert np.all(np.abs(extra - want) <= 2 * (2 ** n - 1) * 9 * U * np.abs(want))
            assert abs(float(extra.sum()) - 160.0) < 1e-9
    finally:
        dev["resident"].free()


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _definition_tail(monkeypatch, n, tol):
    """resolve_multi_prop_csr replaced by the definition: the profile map_main then writes is the expectation."""
    def by_definition(args, taxids2abs, mm, taxid2info):
        glen = [taxid2info[x][0] for x in mm["taxids"]] if args.length_normalize else None
        mmdef.resolve(taxids2abs, mm["taxids"], mm["mm_offsets"], mm["mm_tax"], mm["mm_hitlen"], glen, n, tol)
        return taxids2abs
    monkeypatch.setattr(mp, "resolve_multi_prop_csr", by_definition)


def _abundances(text):
    return [ln.split("\t")[4] for ln in text.splitlines() if ln and ln[0] != "@"]


def _end_to_end(monkeypatch, tmp_path, infile, dbinfo, base_args, golden_cami=None):
    def run(tag, **over):
        out = tmp_path / (tag + ".cami")
        mp.map_main(sc.make_args(str(infile), str(dbinfo), str(out), dict(base_args, **over)))
        return out.read_text()
    plain = run("plain")
    one = run("one", multimap_iterations=1)
    assert one == plain  # byte for byte
    if golden_cami is not None:
        sc._cami_close(plain, golden_cami)
    host = run("host", multimap_iterations=8)
    devc = run("dev", multimap_iterations=8, device_multimap=True)
    one_dev = run("one_dev", multimap_iterations=1, device_multimap=True)
    assert one_dev == run("plain_dev", device_multimap=True)
    with monkeypatch.context() as m:
        _definition_tail(m, 8, 1e-8)
        want = run("want")
    sc._cami_close(host, want)
    sc._cami_close(devc, want)
    assert _abundances(host) != _abundances(plain) and _abundances(devc) != _abundances(plain)
    return want


def _close_strains_sam(nscale=1000):
    """Three taxa and the reads of the hand example (metalign_amd/multimap.py), scaled: unique reads 3 : 1 : 1, as many reads shared by
    A and B as by B and C."""
    dbtext, accs, taxids = samgen.make_dbinfo(seed=7, n_species=12)
    first = {}
    for a, t in zip(accs, taxids):
        first.setdefault(t, a)
    A, B, C = [first[t] for t in sorted(first)[:3]]
    rng = random.Random(3)
    reads = [(A,)] * (3 * nscale // 5) + [(B,)] * (nscale // 5) + [(C,)] * (nscale // 5) + [(A, B)] * (nscale // 2) + [(B, C)] * (nscale // 2)
    rng.shuffle(reads)
    reads = [(A, A)] + reads + [(A,)]  # (the file's first read loses its first line, its last read is never processed)
    out = ["@HD\tVN:1.6\tSO:unsorted\n"]
    for k, hit in enumerate(reads):
        seq = samgen._seq(rng, 40)
        out.append(samgen._line("r%d" % k, 0, hit[0], "40M", seq, 0))
        for other in hit[1:]:
            out.append(samgen._line("r%d" % k, 256, other, "40M", "*", 1))
    return dbtext, "".join(out)


def test_command_line_on_a_sam_and_a_bam_of_three_close_taxa(hip, monkeypatch, tmp_path, capsys):
    dbtext, text = _close_strains_sam()
    assert text.count("\n") > 2000
    dbinfo = tmp_path / "db_info.txt"
    dbinfo.write_text(dbtext)
    sam, bm = tmp_path / "x.sam", tmp_path / "x.bam"
    sam.write_text(text)
    bm.write_bytes(bamgen.sam_to_bam(text, block=20000))
    (tmp_path / "s").mkdir()
    (tmp_path / "b").mkdir()
    base = {"input_type": "AUTO", "sampleID": "s"}
    want_sam = _end_to_end(monkeypatch, tmp_path / "s", sam, dbinfo, base)
    want_bam = _end_to_end(monkeypatch, tmp_path / "b", bm, dbinfo, base)
    assert want_sam == want_bam
    # --verbose tells the iterations, the last change and, on the device, the classes
    capsys.readouterr()
    for over, word in (({}, "iteration(s); last relative change"), ({"device_multimap": True}, "over 2 classes of 1000 reads")):
        mp.map_main(sc.make_args(str(sam), str(dbinfo), str(tmp_path / "v.cami"),
                                 dict(base, verbose=True, multimap_iterations=8, multimap_tol=0.0, **over)))
        said = capsys.readouterr().out
        assert "reassigned in 8 iteration(s)" in said and word in said


def test_command_line_on_a_golden_bulk_case(hip, monkeypatch, tmp_path):
    spec = sc.load_bulk()["single_3k"]
    sam, dbp = sc.materialise_bulk("single_3k", spec, tmp_path)
    run = [r for r in spec["runs"] if r.get("map_main_raises") is None and not r["args"].get("low_mem")][0]
    _end_to_end(monkeypatch, tmp_path, sam, dbp, run["args"], golden_cami=run["cami"])
