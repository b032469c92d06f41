"""--side_reads unique on the device: mg_records_mask_unique_dev against the definition (side_reads.unique_mask_of_records) over
synthetic records and synthetic verdict words, and map_main end to end against the families' definitions over
side_reads.unique_lines."""
import ctypes
import gzip

import numpy as np
import pytest

import bamgen
import collate_cases
import side_reads_cases as src
import stage_c_checks as sc
from metalign_amd import _hip, collate
from metalign_amd import map_and_profile as mp
from metalign_amd import side_outputs as so
from metalign_amd import side_reads as sr

pytestmark = pytest.mark.gpu

T, W = src.TILE, src.SCAN_THREADS
GUARD = 0xA5A5A5A5A5A5A5A5
KEPT0, OUTSIDE0 = 5, 7  # what d_stats2 holds before a call: it is added to


def _mask_on_device(hip, recs, words, ref2tax, in_place=False):
    """One call with guard words behind d_out and d_stats2 -> (the records written, records kept, records outside)."""
    n, nreads, nref = len(recs), len(words) // 2, len(ref2tax)
    guard_rec = np.full(4, 0xA5A5A5A5, dtype=np.uint32).view(_hip.REC_DTYPE)
    d_in = hip.array(np.concatenate([recs, np.repeat(guard_rec, 4)]))
    d_out = d_in if in_place else hip.array(np.repeat(guard_rec, n + 4))
    d_words = hip.array(words if nreads else np.zeros(2, np.uint64))
    d_r2t = hip.array(ref2tax if nref else np.zeros(1, np.uint32))
    d_stats = hip.array(np.array([KEPT0, OUTSIDE0, GUARD, GUARD], dtype=np.uint64))
    try:
        hip._chk(hip.lib.mg_records_mask_unique_dev(ctypes.c_void_p(d_in.ptr), ctypes.c_uint64(n), ctypes.c_void_p(d_words.ptr),
                                                    ctypes.c_uint64(nreads), ctypes.c_void_p(d_r2t.ptr), ctypes.c_uint32(nref),
                                                    ctypes.c_void_p(d_out.ptr), ctypes.c_void_p(d_stats.ptr)))
        hip.sync()
        out, stats = d_out.download(), d_stats.download()
        if not in_place:
            assert d_in.download().tobytes() == np.concatenate([recs, np.repeat(guard_rec, 4)]).tobytes(), "the input was written"
    finally:
        for d in {id(x): x for x in (d_in, d_out, d_words, d_r2t, d_stats)}.values():
            d.free()
    assert out[n:].tobytes() == np.repeat(guard_rec, 4).tobytes(), "written behind d_out"
    assert stats[2] == GUARD and stats[3] == GUARD, "written behind d_stats2"
    return out[:n], int(stats[0]) - KEPT0, int(stats[1]) - OUTSIDE0


def _check(hip, recs, words, ref2tax, in_place=False):
    want = sr.unique_mask_of_records(recs, words, ref2tax)
    out, kept, outside = _mask_on_device(hip, recs, words, ref2tax, in_place)
    # nothing but bit 2048 of flag_len differs, and it is set exactly where the definition masks
    for field in ("ref_new", "matched", "total"):
        assert np.array_equal(out[field], recs[field]), field
    assert np.array_equal(out["flag_len"], recs["flag_len"] | np.where(want, 0, 2048).astype(np.uint32))
    assert kept == int(want.sum())
    assert outside == sr.outside_of_records(recs, words)
    return want, outside


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_the_kernel_against_the_definition(hip, n, in_place):
    want, outside = _check(hip, *src.synthetic(n, seed=100 + n), in_place=in_place)
    assert outside == 0
    if n >= T - 1:
        assert 0.1 * n < want.sum() < 0.5 * n


def test_the_generated_inputs_are_not_vacuous():
    share = src.reasons(*src.synthetic(2 * T + 1, seed=100 + 2 * T + 1))
    assert share["kept"] >= 0.10 and share["kind"] >= 0.05 and share["dropped"] >= 0.05 and share["taxon"] >= 0.05, share


@pytest.mark.parametrize("in_place", [False, True])
def test_more_tiles_than_the_scan_workgroup_has_threads(hip, in_place):
    n = (W + 1) * T + 5
    want, outside = _check(hip, *src.synthetic(n, seed=7), in_place=in_place)
    assert outside == 0 and 0.1 * n < want.sum() < 0.5 * n
    assert want[W * T:].sum() > 100  # (records whose tile base comes from the scan's second round)


def test_every_record_new_and_one_read_across_every_tile(hip):
    n = 3 * T + 7
    recs, words, ref2tax = src.synthetic(n, seed=8, p_new=2.0)
    want, _ = _check(hip, recs, words, ref2tax)
    assert len(words) == 2 * n and want.sum() > 0.1 * n
    recs, words, ref2tax = src.synthetic(n, seed=9, p_new=0.0)
    assert len(words) == 2
    words[0] = 1 | (1 << 2)  # the one read is unique, for taxon 1
    want, _ = _check(hip, recs, words, ref2tax)
    assert not want[0] and 0.3 * n < want.sum() < 0.7 * n and want[-3 * 64:].any()
    words[0] = 2
    assert not _check(hip, recs, words, ref2tax)[0].any()


def test_reads_that_start_on_a_wavefronts_last_lane_and_a_tiles_last_record(hip):
    n = 2 * T + 130
    starts = [0, 63, 64 * 5 + 63, 1023, 1024, T - 1, T, 2 * T - 1, 2 * T + 63, 2 * T + 129]
    recs, _, ref2tax = src.synthetic(n, seed=10, p_new=0.0)
    recs["ref_new"] &= np.uint32(_hip.REF_MASK)
    recs["ref_new"][starts] |= np.uint32(_hip.NEW_BIT)
    for kinds in ([1] * len(starts), [1, 0, 1, 1, 0, 1, 2, 1, 3, 1]):
        words = np.zeros(2 * len(starts), dtype=np.uint64)
        words[0::2] = [k | (((r % 2) << 2) if k == 1 else 0) for r, k in enumerate(kinds)]
        want, outside = _check(hip, recs, words, ref2tax)
        assert outside == 0 and not want[0] and want.any()
        if 0 not in kinds:  # (every read unique, the taxa alternating: about half of the records are kept, in every read)
            assert all(want[a:b].any() for a, b in zip(starts[1:-1], starts[2:]) if b - a > 16)


def test_words_one_read_short_and_records_in_front_of_the_first_read(hip):
    recs, words, ref2tax = src.synthetic(2 * T + 1, seed=11)
    want, outside = _check(hip, recs, words[:-2], ref2tax)
    assert outside >= 1
    _, outside = _check(hip, recs, words[:0], ref2tax)
    assert outside == len(recs)
    recs, words, ref2tax = src.synthetic(T + 9, seed=12, first_new=False, p_new=0.01)
    first = int(np.flatnonzero(recs["ref_new"] & np.uint32(_hip.NEW_BIT))[0])
    want, outside = _check(hip, recs, words, ref2tax)
    assert first > 0 and outside == first and not want[:first].any()
    _check(hip, recs, words, ref2tax[:0])  # every row at or above nref
    _check(hip, recs, words, ref2tax[:3])


def test_the_wrapper_counts_and_refuses_the_words_of_another_stream(hip):
    recs, words, ref2tax = src.synthetic(5000, seed=13)
    want = sr.unique_mask_of_records(recs, words, ref2tax)
    d_recs, d_words, d_r2t = hip.array(recs), hip.array(words), hip.array(ref2tax)
    try:
        assert hip.records_mask_unique(d_recs.ptr, len(recs), d_words.ptr, len(words) // 2, d_r2t.ptr, len(ref2tax), d_recs.ptr) \
            == (int(want.sum()), 0)
        with pytest.raises(_hip.HipError, match="belong to no read"):
            hip.records_mask_unique(d_recs.ptr, len(recs), d_words.ptr, len(words) // 2 - 1, d_r2t.ptr, len(ref2tax), d_recs.ptr)
        assert hip.records_mask_unique(d_recs.ptr, 0, d_words.ptr, 0, d_r2t.ptr, 0, d_recs.ptr) == (0, 0)
        with pytest.raises(_hip.HipError):  # (the records are read and written 16 bytes at a time)
            hip.records_mask_unique(d_recs.ptr + 4, 10, d_words.ptr, len(words) // 2, d_r2t.ptr, len(ref2tax), d_recs.ptr + 4)
    finally:
        for d in (d_recs, d_words, d_r2t):
            d.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
FILES = ("coverage", "depth", "depth_windows", "identity")
WINDOW = 500


def _definitions(d, tag, lines, dbinfo, unique):
    """The four files as the definitions give them: over `lines`, or over side_reads.unique_lines of them."""
    (d / tag).mkdir()
    paths = {k: str(d / tag / (k + ".tsv")) for k in FILES}
    args = sc.make_args("x.sam", dbinfo, "-", dict(paths, depth_window_size=WINDOW, **({"side_reads": "unique"} if unique else {})))
    acc2info, taxid2info = mp.get_acc2info(args)
    so.write_headers(args)
    feed = (lambda: sr.unique_lines(lines, acc2info, args.pct_id)) if unique else (lambda: lines)
    so.SideOutputs.of(args, "x.sam").append_from_definition("x.sam", feed, acc2info, taxid2info)
    return {k: open(p, "rb").read() for k, p in paths.items()}


def _run(path, dbinfo, tmp_path, tag, mode, **extra):
    (tmp_path / tag).mkdir()
    paths = {k: str(tmp_path / tag / (k + ".tsv")) for k in FILES}
    out = tmp_path / tag / "out.cami"
    ov = dict(paths, input_type="sam", db="unused.fna", sampleID="s", depth_window_size=WINDOW, **extra)
    if mode is not None:
        ov["side_reads"] = mode
    mp.map_main(sc.make_args(str(path), dbinfo, str(out), ov))
    return out.read_bytes(), {k: open(p, "rb").read() for k, p in paths.items()}


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("side_reads")
    dbtext, lines = src.sample()
    dbinfo = str(d / "db_info.txt")
    open(dbinfo, "w").write(dbtext)
    text = "".join(lines)
    (d / "s.sam").write_text(text)
    (d / "s.sam.gz").write_bytes(gzip.compress(text.encode()))
    (d / "s.bam").write_bytes(bamgen.sam_to_bam(text, block=20000))
    shuffled = collate_cases.coordinate_shuffle(text)
    (d / "sorted.sam").write_text("".join(shuffled))
    want = dict(all=_definitions(d, "want_all", lines, dbinfo, False), unique=_definitions(d, "want_unique", lines, dbinfo, True),
                sorted_all=_definitions(d, "want_sorted_all", shuffled, dbinfo, False),
                sorted_unique=_definitions(d, "want_sorted_unique", list(collate.collated_lines(shuffled)), dbinfo, True))
    return d, dbinfo, want


def _rows_of(coverage_bytes):
    """{accession: alignments} of a coverage file's S rows."""
    return {f[1]: int(f[4]) for f in (ln.split("\t") for ln in coverage_bytes.decode().splitlines()) if f[0] == "S"}


def test_the_case_the_feature_exists_for(sample):
    _, _, want = sample
    every, unique = _rows_of(want["all"]["coverage"]), _rows_of(want["unique"]["coverage"])
    assert every[src.RELATIVE] > 0 and src.RELATIVE not in unique and set(unique) == set(src.ACCS[:4])
    assert all(0 < unique[a] < every[a] for a in unique)
    for k in FILES:
        head = want["all"][k].split(b"\n", 1)[0] + b"\n"
        assert want["unique"][k].startswith(head + b"#reads\tunique\n") and b"#reads" not in want["all"][k]


@pytest.mark.parametrize("form", ["s.sam", "s.sam.gz", "s.bam"])
def test_map_main_in_both_modes(hip, sample, tmp_path, form):
    d, dbinfo, want = sample
    cami_u, got_u = _run(d / form, dbinfo, tmp_path, "unique", "unique")
    cami_a, got_a = _run(d / form, dbinfo, tmp_path, "all", "all")
    cami_0, got_0 = _run(d / form, dbinfo, tmp_path, "default", None)
    assert got_u == want["unique"]
    assert got_a == want["all"] and got_0 == want["all"]
    assert cami_u == cami_a == cami_0 and cami_u.count(b"\n") > 8


def test_map_main_the_whole_text_in_one_call(hip, sample, tmp_path, monkeypatch):
    d, dbinfo, want = sample
    monkeypatch.setenv("MG_NO_STREAM", "1")
    cami_u, got_u = _run(d / "s.sam", dbinfo, tmp_path, "unique", "unique")
    cami_a, got_a = _run(d / "s.sam", dbinfo, tmp_path, "all", "all")
    assert got_u == want["unique"] and got_a == want["all"] and cami_u == cami_a


def test_map_main_with_read_assignments(hip, sample, tmp_path):
    d, dbinfo, want = sample
    for form in ("s.sam", "s.bam"):
        rows_u, rows_a = tmp_path / (form + ".u.tsv"), tmp_path / (form + ".a.tsv")
        cami_u, got_u = _run(d / form, dbinfo, tmp_path, form + "_unique", "unique", read_assignments=str(rows_u))
        cami_a, got_a = _run(d / form, dbinfo, tmp_path, form + "_all", "all", read_assignments=str(rows_a))
        assert got_u == want["unique"] and got_a == want["all"] and cami_u == cami_a
        assert rows_u.read_bytes() == rows_a.read_bytes() and rows_u.read_bytes().count(b"\tU\t") > 1000


def test_map_main_a_coordinate_sorted_file_collated(hip, sample, tmp_path):
    d, dbinfo, want = sample
    (tmp_path / "sorted.bam").write_bytes(bamgen.sam_to_bam((d / "sorted.sam").read_text(), block=20000))
    for path in (d / "sorted.sam", tmp_path / "sorted.bam"):
        rows = tmp_path / (path.name + ".rows.tsv")
        cami_u, got_u = _run(path, dbinfo, tmp_path, path.name + "_unique", "unique", collate="always")
        cami_a, got_a = _run(path, dbinfo, tmp_path, path.name + "_all", "all", collate="always")
        assert got_u == want["sorted_unique"] and got_a == want["sorted_all"] and cami_u == cami_a
        _, got_r = _run(path, dbinfo, tmp_path, path.name + "_rows", "unique", collate="always", read_assignments=str(rows))
        assert got_r == want["sorted_unique"] and rows.stat().st_size > 1000
