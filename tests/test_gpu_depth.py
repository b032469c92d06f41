"""-m gpu: --depth / --depth_windows on the device — the depth kernels (mg_depth.hip) and the command line.  The expectation is
always metalign_amd/depth.py over the same records / lines."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import bamgen
import collate_cases
import coverage_cases as cc
import side_bins_cases as sb
import stage_c_checks as sc
from metalign_amd import _hip
from metalign_amd import coverage as cv
from metalign_amd import depth as dp
from metalign_amd import map_and_profile as mp

pytestmark = pytest.mark.gpu

PCT = 0.5
TILE = 1024  # mg_depth_core.h: kTile, the slots of a scan tile
GUARD64, GUARD32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5
# an accession owns L + 1 slots: t1023 fills tile 0 exactly (a1 starts ON a tile edge), a1 .. a33 end inside tile 1; two
# accessions without a base lie between others
NAMES = ["t1023", "a1", "z0", "a31", "a33", "z1", "big", "huge"]
LENGTHS = {"t1023": 1023, "a1": 1, "z0": 0, "a31": 31, "a33": 33, "z1": 0, "big": 100000, "huge": 3 << 20}
ROW = {a: i for i, a in enumerate(NAMES)}
SMALL = NAMES[:7]


def _rec(row, matched, total, flag=0, new=0):
    return (row | (new << 31), matched, total, flag | (40 << 12))


def _edge_pairs():
    """(record, place) pairs that start and end on every edge of the scan's tiles, stop at L, run past it, sit on L - 1 and on
    L, have no span, do not count, lie on accessions of length 0 and on a row that does not exist."""
    out = []
    big, L = ROW["big"], LENGTHS["big"]
    for b in (0, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE):     # (slots from the accession's start)
        for e in (1, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1):
            if e > b:
                out.append((_rec(big, 9, 10), (b, e - b)))
    # big starts at slot 1097: the intervals that start and end on the tile edges of the whole array
    first = sum(LENGTHS[a] + 1 for a in NAMES[:ROW["big"]])
    for edge in (2 * TILE, 5 * TILE):
        for b in (edge - first - 1, edge - first, edge - first + 1):
            out += [(_rec(big, 9, 10), (b, 1)), (_rec(big, 9, 10), (b, TILE)), (_rec(big, 9, 10), (b - 40, 40))]
    out += [(_rec(big, 5, 10), (L - 40, 40)), (_rec(big, 5, 10), (L - 40, 41)), (_rec(big, 5, 10), (L - 7, 4000)),  # at L, past L
            (_rec(big, 5, 10), (L - 1, 1)), (_rec(big, 5, 10), (L - 1, 50)), (_rec(big, 5, 10), (L, 10)),         # L - 1, and L: unplaced
            (_rec(big, 5, 10), (1000, 0)),                                                                        # span 0: unplaced
            (_rec(big, 4, 10), (2000, 10)), (_rec(big, 10, 10, flag=2048), (2000, 10)),                           # do not count
            (_rec(big, 10, 10, flag=256, new=1), (3000, 10)),                                                     # a secondary counts
            (_rec(ROW["t1023"], 1, 1), (0, 1023)), (_rec(ROW["t1023"], 1, 1), (1022, 1)), (_rec(ROW["t1023"], 1, 1), (1022, 9)),
            (_rec(ROW["t1023"], 1, 1), (1023, 1)),
            (_rec(ROW["a1"], 1, 1), (0, 1)), (_rec(ROW["a1"], 1, 1), (0, 40)), (_rec(ROW["a1"], 1, 1), (1, 1)),
            (_rec(ROW["z0"], 1, 1), (0, 1)), (_rec(ROW["z1"], 1, 1), (0, 7)),                                     # no base: unplaced
            (_rec(ROW["a31"], 1, 1), (0, 31)), (_rec(ROW["a31"], 1, 1), (30, 5)), (_rec(ROW["a31"], 1, 1), (31, 1)),
            (_rec(ROW["a31"], 1, 1), (3, 4)),
            (_rec(ROW["a33"], 1, 1), (0, 33)), (_rec(ROW["a33"], 1, 1), (31, 2)), (_rec(ROW["a33"], 1, 1), (32, 1)),
            (_rec(ROW["a33"], 1, 1), (33, 1)), (_rec(ROW["a33"], 1, 1), (5, 2 ** 32 - 1)),
            (_rec(len(NAMES) + 3, 1, 1), (0, 5)), (_rec(0x7FFFFFFF, 1, 1), (0, 5))]                               # rows >= nacc: unplaced
    return out


def _arrays(pairs):
    recs = np.array([p[0] for p in pairs], dtype=_hip.REC_DTYPE) if pairs else np.zeros(0, dtype=_hip.REC_DTYPE)
    places = np.array([p[1] for p in pairs], dtype=_hip.PLACE_DTYPE) if pairs else np.zeros(0, dtype=_hip.PLACE_DTYPE)
    return recs, places


def _generated(n, seed=3):
    rng = np.random.default_rng(seed)
    edge = _edge_pairs()
    pairs = []
    for i in range(n):
        if i % 3 == 0:
            pairs.append(edge[(i // 3) % len(edge)])
        else:
            row = int(rng.integers(0, len(SMALL)))
            L = LENGTHS[NAMES[row]]
            pairs.append((_rec(row, int(rng.integers(3, 11)), 10, flag=int(rng.choice([0, 16, 256, 2048, 99])), new=int(rng.integers(0, 2))),
                          (int(rng.integers(0, L + 3)), int(rng.choice([0, 1, 31, 32, 33, 40, 150, 5000])))))
    return pairs


def _guarded_results(hip, dev):
    """mg_depth_finish and both fetches into arrays with guard words behind them -> what Depth.result() gives."""
    n = dev.nacc
    aln = np.full(n + 4, GUARD64, dtype=np.uint64)
    unplaced, nrows, nwin = ctypes.c_uint64(GUARD64), ctypes.c_uint64(GUARD64), ctypes.c_uint64(GUARD64)
    hip._chk(hip.lib.mg_depth_finish(dev.handle, _hip._np(aln, ctypes.c_uint64), ctypes.byref(unplaced), ctypes.byref(nrows),
                                     ctypes.byref(nwin)))
    nrows, nwin = int(nrows.value), int(nwin.value)
    assert nrows <= n and np.all(aln[n:] == GUARD64), "written behind the alignments"
    acc = np.full(nrows + 4, GUARD32, dtype=np.uint32)
    hist = np.full(nrows * _hip.DEPTH_BINS + 4, GUARD64, dtype=np.uint64)
    hip._chk(hip.lib.mg_depth_fetch_rows(dev.handle, _hip._np(acc, ctypes.c_uint32), _hip._np(hist, ctypes.c_uint64)))
    assert np.all(acc[nrows:] == GUARD32) and np.all(hist[nrows * _hip.DEPTH_BINS:] == GUARD64), "written behind the rows"
    win = np.zeros(nwin + 2, dtype=_hip.DEPTH_WINDOW_DTYPE)
    win.view(np.uint8)[:] = 0xA5
    hip._chk(hip.lib.mg_depth_fetch_windows(dev.handle, ctypes.c_void_p(win.ctypes.data)))
    assert np.all(win[nwin:].view(np.uint8) == 0xA5), "written behind the windows"
    hist = hist[:nrows * _hip.DEPTH_BINS].reshape(nrows, _hip.DEPTH_BINS)
    per = {int(a): {int(c): int(hist[r, c]) for c in np.flatnonzero(hist[r])} for r, a in enumerate(acc[:nrows])}
    windows = {}
    for a, j, s, c in zip(win["acc"][:nwin].tolist(), win["index"][:nwin].tolist(), win["depth_sum"][:nwin].tolist(),
                          win["covered"][:nwin].tolist()):
        windows.setdefault(a, []).append((j, s, c))
    return aln[:n], int(unplaced.value), per, windows


def _check(hip, calls, names=NAMES, pct=PCT, windows=(0, 7), lengths=LENGTHS):
    """The device over `calls` (lists of pairs, one add_dev each) against the definition over all of them, per window width."""
    lens = {a: lengths[a] for a in names}
    recs, places = _arrays([p for pairs in calls for p in pairs])
    want = None
    for W in windows:
        dev = hip.depth([lens[a] for a in names], W)
        try:
            for pairs in calls:
                dev.add(*_arrays(pairs), pct)
            aln, unplaced, per, win = _guarded_results(hip, dev)
        finally:
            dev.free()
        want = dp.depth_of_records(recs, places, names, lens, pct, W)
        assert {names[r]: [int(aln[r]), H] for r, H in per.items()} == want.per, W
        assert all(int(aln[i]) == 0 for i in range(len(names)) if i not in per)
        assert unplaced == want.unplaced, W
        assert {names[r]: w for r, w in win.items()} == want.windows, W
        for a, H in want.per.items():
            assert sum(H[1].values()) == lens[a]
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_add_dev_from_arrays_histograms_and_windows(hip, n):
    want = _check(hip, [_generated(n)], names=SMALL, windows=(1, 7, 32, 1000))
    if n == 4097:
        assert set(want.per) == set(SMALL) - {"z0", "z1"} and want.unplaced > 100
        assert max(want.per["a1"][1]) > 5 and len(want.windows["big"]) > 50
        # W = 1 is the per-base depth itself
        base = dp.depth_of_records(*_arrays(_generated(n)), SMALL, LENGTHS, PCT, 1)
        assert sum(w[1] for w in base.windows["a33"]) == sum(c * k for c, k in base.per["a33"][1].items())


def test_every_edge_case_alone_and_together(hip):
    edge = _edge_pairs()
    want = _check(hip, [edge], names=SMALL, windows=(1, 1000))
    assert want.unplaced >= 10 and set(want.per) == {"t1023", "a1", "a31", "a33", "big"}
    for p in edge:
        _check(hip, [[p]], names=SMALL, windows=(7,))


@pytest.mark.parametrize("grid", [0, 2])
def test_one_long_alignment_among_short_ones_few_workgroups(hip, grid):
    rng = np.random.default_rng(9)
    huge = ROW["huge"]
    pairs = [(_rec(huge, 10, 10), (int(p), 40)) for p in rng.integers(0, LENGTHS["huge"] - 40, 4000)]
    pairs.insert(1777, (_rec(huge, 10, 10), (12345, 1 << 20)))
    pairs += _generated(300)
    _hip.debug_set("depth_grid", grid)
    try:
        want = _check(hip, [pairs], windows=(0, 1000))
    finally:
        _hip.debug_set("depth_grid", 0)
    assert want.per["huge"][0] == 4001 and sum(k for c, k in want.per["huge"][1].items() if c) > (1 << 20)
    assert len(want.windows["huge"]) > 1048


@pytest.mark.parametrize("grid", [1, 3])
def test_more_accessions_than_lds_bins_add_to_memory_directly(hip, grid):
    """3000 accessions through the 1024 bins of one workgroup (and of three): at least 1976 of them find no slot, whatever the hash
    does, and add their alignments to memory directly — in the launch that counts the unplaced."""
    assert sb.overflows("mg_depth.hip", "kBins") >= 1000
    rng = np.random.default_rng(12)
    pairs = [(_rec(row, 10, 10), (sb.LENGTH, 9) if i % 97 == 5 else (int(rng.integers(0, 60)), int(rng.integers(1, 40))))
             for i, row in enumerate(sb.rows())]
    _hip.debug_set("depth_grid", grid)
    try:
        assert _hip.debug_get("depth_grid") == grid
        want = _check(hip, [pairs], names=sb.NAMES, windows=(16,), lengths=dict.fromkeys(sb.NAMES, sb.LENGTH))
    finally:
        _hip.debug_set("depth_grid", 0)
    assert len(want.per) > sb.NACC - 70 and want.unplaced >= 2 * len(sb.BEYOND) + 50  # (some accessions' only record is unplaced)


def test_intervals_on_both_sides_of_a_step_of_the_tile_scan(hip):
    """One accession of 4 300 000 bases: 4200 tiles for the one workgroup that scans 4096 tile sums in a step, so the depth behind
    slot 4096 * 1024 comes out right only with the carry across the step."""
    L, edge = 4300000, 4096 * TILE
    assert (L + 1 + TILE - 1) // TILE > 4096
    pairs = [(_rec(0, 10, 10), place) for place in
             [(100, 50), (edge - 3000, 2000), (edge - 20, 40), (edge - 1, 1), (edge, 5), (edge, 1), (edge + 1, 2000),
              (edge - 200000, 300000), (L - 10, 100), (L - 1, 1), (0, 1)] + [(edge - 7, 14)] * 5]
    want = _check(hip, [pairs], names=["long"], windows=(1000,), lengths={"long": L})
    assert want.per["long"][0] == 16 and max(want.per["long"][1]) == 9 and want.unplaced == 0  # (nine deep at slot `edge`)
    assert {j for j, _, _ in want.windows["long"]} >= {0, edge // 1000 - 1, edge // 1000, edge // 1000 + 1, (L - 1) // 1000}


def test_identical_intervals_contend_and_cross_the_clamp(hip):
    big = ROW["big"]
    want = _check(hip, [[(_rec(big, 10, 10), (1234, 20))] * 2000 + [(_rec(big, 10, 10), (5000, 30))] * 5000], windows=(0, 16))
    assert want.per == {"big": [7000, {0: 100000 - 50, 2000: 20, dp.CAP: 30}]}
    assert (5000 // 16, 5000 * (16 - 5000 % 16), 16 - 5000 % 16) in want.windows["big"]  # the sum is not clamped


def test_two_and_three_calls_equal_one_and_an_add_after_finish_is_refused(hip):
    pairs = _generated(1500, seed=5)
    a = _check(hip, [pairs])
    b = _check(hip, [pairs[:700], pairs[700:]])
    c = _check(hip, [pairs[:700], [], pairs[700:1100], pairs[1100:]])
    assert a == b == c
    dev = hip.depth([LENGTHS[x] for x in NAMES], 5)
    try:
        dev.add(*_arrays(pairs[:10]), PCT)
        dev.finish()
        for late in (pairs[:3], []):
            with pytest.raises(_hip.HipError) as e:
                dev.add(*_arrays(late), PCT)
            assert e.value.code == _hip.ERR_STATE
        dev.fetch_rows()
        with pytest.raises(_hip.HipError) as e:
            dev.fetch_rows()
        assert e.value.code == _hip.ERR_STATE
    finally:
        dev.free()


def test_no_accession_and_only_empty_accessions(hip):
    for W in (0, 3):
        dev = hip.depth([], W)
        try:
            dev.add(*_arrays([(_rec(0, 1, 1), (0, 1))]), PCT)
            aln, unplaced, per, win = dev.result()
            assert len(aln) == 0 and unplaced == 1 and per == {} and win == {}
        finally:
            dev.free()
    dev = hip.depth([0, 0, 5, 0], 2)
    try:
        dev.add(*_arrays([(_rec(0, 1, 1), (0, 1)), (_rec(2, 1, 1), (4, 9)), (_rec(3, 1, 1), (0, 1)), (_rec(9, 1, 1), (0, 1))]), PCT)
        aln, unplaced, per, win = dev.result()
        assert list(aln) == [0, 0, 1, 0] and unplaced == 3 and per == {2: {0: 4, 1: 1}} and win == {2: [(2, 1, 1)]}
    finally:
        dev.free()


def test_slot_offsets_beyond_32_bits(hip):
    """Three accessions of 2^31 - 1 bases (25.8 GB of slots): the third one's slots lie beyond slot 2^32."""
    free, _, pooled = hip.mem_info()
    if free + pooled < (64 << 30):
        pytest.skip("mem_info() shows less than 64 GB free: the 25.8 GB of slots are not tried")
    L = 2 ** 31 - 1
    names = ["x", "y", "z"]
    lengths = dict.fromkeys(names, L)
    rng = np.random.default_rng(4)
    pairs = []
    for row in range(3):
        for _ in range(12):
            pairs.append((_rec(row, 10, 10), (int(L - 1 - rng.integers(0, 1000)), int(rng.integers(1, 300)))))
            pairs.append((_rec(row, 10, 10), (int(rng.integers(0, 1000)), int(rng.integers(1, 300)))))
        pairs.append((_rec(row, 10, 10), (L - 1, 7)))
        pairs.append((_rec(row, 10, 10), (0, 33 + row)))
        pairs.append((_rec(row, 10, 10), (999990, 20 + row)))  # across the first window edge
    try:
        want = _check(hip, [pairs], names=names, windows=(1000000,), lengths=lengths)
    finally:
        hip.mem_trim()
    assert want.unplaced == 0 and all(want.per[a][0] == 27 and len(want.windows[a]) == 3 for a in names)
    assert want.windows["z"][-1][0] == (L - 1) // 1000000


# ---- end to end ---------------------------------------------------------------------------------------------------------------
W_E2E = 100


def _tables(dbinfo_path):
    return mp.get_acc2info(sc.make_args("-", dbinfo_path, "-", {}))


def _definition_bytes(lines, dbinfo_path, source=None, header=True, window=W_E2E):
    acc2info, taxid2info = _tables(dbinfo_path)
    got = dp.depth(lines, acc2info, 0.5, window)
    return (((dp.HEADER if header else "") + dp.format_block(dp.rows(got, acc2info, taxid2info), got.unplaced, source)).encode(),
            ((dp.WINDOWS_HEADER if header else "") + dp.format_window_block(dp.window_rows(got, acc2info), source)).encode())


def _run(sam, dbinfo, tmp_path, tag, depth=True, **extra):
    """map_main -> (profile text, (depth file, windows file) or None)."""
    out, dep, win = tmp_path / (tag + ".cami"), tmp_path / (tag + ".depth.tsv"), tmp_path / (tag + ".win.tsv")
    ov = dict({"input_type": "AUTO", "sampleID": "s"}, **extra)
    if depth:
        ov.update(depth=str(dep), depth_windows=str(win), depth_window_size=W_E2E)
    mp.map_main(sc.make_args(str(sam), str(dbinfo), str(out), ov))
    return out.read_text(), ((dep.read_bytes(), win.read_bytes()) if depth else None)


def _dressed(sam_path, dbinfo_path, seed):
    acc2info, _ = cc.tables(open(dbinfo_path).read())
    accs = [a for a in acc2info if a != "Unmapped"]
    return cc.dress(open(sam_path).read(), accs, acc2info, seed)


def _three_forms(d, stem, lines):
    text = "".join(lines)
    (d / (stem + ".sam")).write_text(text)
    (d / (stem + ".sam.gz")).write_bytes(gzip.compress(text.encode()))
    (d / (stem + ".bam")).write_bytes(bamgen.sam_to_bam(text, block=20000))
    return [d / (stem + ".sam"), d / (stem + ".sam.gz"), d / (stem + ".bam")]


def _chunked(path, dbinfo, tmp_path, tag):
    """The file's lines through the chunked map_and_process, as the product does when the device path declines a file."""
    dep, win = tmp_path / (tag + ".chunked.tsv"), tmp_path / (tag + ".chunked.win.tsv")
    args = sc.make_args(str(path), str(dbinfo), str(tmp_path / (tag + ".c.cami")),
                        {"depth": str(dep), "depth_windows": str(win), "depth_window_size": W_E2E})
    acc2info, taxid2info = mp.get_acc2info(args)

    def stream():
        if path.name.endswith(".bam"):
            return None, mp.bam.sam_lines(str(path))
        fh = gzip.open(path, "rb") if path.name.endswith(".gz") else open(path, "rb")
        return fh, fh
    dp.write_depth(str(dep))
    dp.write_windows(str(win))
    fh, lines = stream()
    t2a, mm, _ = mp.map_and_process(args, lines, acc2info, taxid2info, _depth=str(path))
    if fh:
        fh.close()
    fh, lines = stream()
    t2a0, mm0, _ = mp.map_and_process(args, lines, acc2info, taxid2info)
    if fh:
        fh.close()
    assert t2a == t2a0 and mm == mm0, tag
    return dep.read_bytes(), win.read_bytes()


def _every_mode(d, stem, lines, dbinfo, tmp_path, monkeypatch):
    """One file as .sam, .sam.gz and .bam — default, many pieces, whole text, the chunked path, and (the lines in coordinate
    order) with --collate always; once with --coverage and --read_assignments beside the two depth files.  In every case both
    depth files are the definition's bytes and everything else is what the run without the new flags writes."""
    want = _definition_bytes(lines, dbinfo)
    forms = _three_forms(d, stem, lines)
    kw = dict(input_type="sam", db="unused.fna")

    def both(path, tag, **more):
        cami, got = _run(path, dbinfo, tmp_path, tag, **kw, **more)
        cami0, none = _run(path, dbinfo, tmp_path, tag + "_0", depth=False, **kw, **more)
        assert none is None and cami == cami0, (tag, path.name)
        return got

    plain = {}
    for path in forms:
        assert both(path, "default") == want, path.name
        plain[path] = (tmp_path / "default_0.cami").read_text()
    # all four outputs together: the coverage file and the assignment rows are those of the run without the depth flags
    path = forms[0]
    cov, rows, cov0, rows0 = (tmp_path / n for n in ("all.cov.tsv", "all.reads.tsv", "all0.cov.tsv", "all0.reads.tsv"))
    cami, got = _run(path, dbinfo, tmp_path, "all", coverage=str(cov), read_assignments=str(rows), **kw)
    cami0, _ = _run(path, dbinfo, tmp_path, "all0", depth=False, coverage=str(cov0), read_assignments=str(rows0), **kw)
    assert got == want and cami == cami0 == plain[path]
    assert cov.read_bytes() == cov0.read_bytes() and rows.read_bytes() == rows0.read_bytes() and len(rows.read_bytes()) > 100
    with monkeypatch.context() as m:
        m.setenv("MG_STREAM_CHUNK_BYTES", str(1 << 16))  # many pieces
        for path in forms:
            assert both(path, "pieces") == want, path.name
    with monkeypatch.context() as m:
        m.setenv("MG_NO_STREAM", "1")  # the whole text in one tokeniser call (a compressed file is streamed all the same)
        for path in forms:
            if path.name.endswith(".gz"):  # (without a placed batch the whole-text call is handed the compressed bytes)
                cami, got = _run(path, dbinfo, tmp_path, "whole", **kw)
                assert got == want and cami == plain[path], path.name
            else:
                assert both(path, "whole") == want, path.name
    with monkeypatch.context() as m:
        m.setattr(mp, "_CHUNK_BYTES", 40000)  # many chunks
        for path in forms:
            assert _chunked(path, dbinfo, tmp_path, path.name) == want, path.name
    shuffled = collate_cases.coordinate_shuffle("".join(lines))  # (POS drawn anew, the lines in coordinate order)
    want_s = _definition_bytes(shuffled, dbinfo)
    for path in _three_forms(tmp_path, stem + "_shuffled", shuffled):
        assert both(path, "col", collate="always") == want_s, path.name
    return forms, want, want_s


@pytest.mark.parametrize("name", ["cascade_break", "paired_mix", "multimap_split", "species_and_virus"])
def test_map_main_hand_cases_in_every_form_and_mode(hip, tmp_path, monkeypatch, name):
    cdir = os.path.join(sc.GOLDEN, "cases")
    dbinfo = os.path.join(cdir, "dbinfo.txt")
    lines = _dressed(os.path.join(cdir, name + ".sam"), dbinfo, 31)
    forms, want, want_s = _every_mode(tmp_path, name, lines, dbinfo, tmp_path, monkeypatch)
    assert want[0].count(b"\nS\t") >= 1 and want[0].count(b"\nG\t") >= 1 and want[1].count(b"\n") >= 2


@pytest.fixture(scope="module")
def bulk(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_bulk")
    sam, dbinfo = sc.materialise_bulk("paired_2k", sc.load_bulk()["paired_2k"], d)
    lines = _dressed(sam, dbinfo, 32)
    forms = _three_forms(d, "b", lines)
    return d, forms, dbinfo, lines, _definition_bytes(lines, dbinfo)


def test_map_main_bulk_in_every_form_and_mode(hip, bulk, tmp_path, monkeypatch):
    d, forms, dbinfo, lines, want = bulk
    assert want[0].count(b"\n") > 20 and int(want[0].rsplit(b"\t", 1)[1]) > 50 and want[1].count(b"\n") > 100
    _, got_want, want_s = _every_mode(tmp_path, "bulk", lines, dbinfo, tmp_path, monkeypatch)
    assert got_want == want and want_s[0].count(b"\n") > 20


def test_either_file_alone_and_without_coverage(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, want = bulk
    for key, i in (("depth", 0), ("depth_windows", 1)):
        out, f = tmp_path / (key + ".cami"), tmp_path / (key + ".tsv")
        mp.map_main(sc.make_args(str(forms[0]), str(dbinfo), str(out), {"input_type": "AUTO", key: str(f), "depth_window_size": W_E2E}))
        assert f.read_bytes() == want[i]
    assert sorted(os.listdir(tmp_path)) == ["depth.cami", "depth.tsv", "depth_windows.cami", "depth_windows.tsv"]  # nothing else
    # the default window is 1000 bases
    f = tmp_path / "w1000.tsv"
    mp.map_main(sc.make_args(str(forms[0]), str(dbinfo), str(tmp_path / "w.cami"), {"input_type": "AUTO", "depth_windows": str(f)}))
    assert f.read_bytes() == _definition_bytes(lines, dbinfo, window=1000)[1]


def test_two_input_files_give_two_blocks(hip, bulk, tmp_path):
    d, forms, dbinfo, lines, want = bulk
    out, dep, win = tmp_path / "two.cami", tmp_path / "two.tsv", tmp_path / "two.win.tsv"
    args = sc.make_args(str(forms[0]), str(dbinfo), str(out), {"input_type": "AUTO", "depth": str(dep), "depth_windows": str(win),
                                                               "depth_window_size": W_E2E})
    args.infiles = [str(forms[0]), str(forms[2])]
    mp.map_main(args)
    one, two = _definition_bytes(lines, dbinfo, source=str(forms[0])), _definition_bytes(lines, dbinfo, source=str(forms[2]), header=False)
    assert dep.read_bytes() == one[0] + two[0] and win.read_bytes() == one[1] + two[1]


def test_a_chunk_the_host_tokeniser_takes_brings_its_depth(hip, bulk, tmp_path, monkeypatch):
    """FLAG 1_6 is 16 to Python's int() and no number to the device parser: that chunk goes through the host tokeniser, and its
    places through coverage.placement."""
    d, forms, dbinfo, lines, _ = bulk
    body = [i for i, ln in enumerate(lines) if cv.retained_fields(ln) is not None]
    odd = list(lines)
    for i in (body[len(body) // 2], body[-3]):
        f = odd[i].split("\t")
        f[1] = "1_6"
        odd[i] = "\t".join(f)
    sam = tmp_path / "odd.sam"
    sam.write_text("".join(odd))
    want = _definition_bytes(odd, dbinfo)
    monkeypatch.setattr(mp, "_CHUNK_BYTES", 40000)
    cami, got = _run(sam, dbinfo, tmp_path, "odd")
    assert got == want
    assert cami == _run(sam, dbinfo, tmp_path, "odd0", depth=False)[0]
