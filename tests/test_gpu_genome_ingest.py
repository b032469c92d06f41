"""-m gpu: organism FASTA files parsed on the device (metalign_amd/csrc/mg_genome.hip, the file driver of mg_stream.hip) and
`build_db --ingest device`.

The definition is build_db.genome_bases: every expected genome is what it returns for the file at hand (tests/genome_cases.py),
and a table built with --ingest device is, file for file and byte for byte, the one --ingest host writes."""
import ctypes
import filecmp
import gzip
import os

import numpy as np
import pytest

import bamgen
import genome_cases as gc
from metalign_amd import _hip, build_db

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def wanted(tmp_path_factory):
    gc.self_check()
    return {name: gc.expected(files, tmp_path_factory.mktemp("want_" + name)) for name, files in gc.CASES.items()}


def _peek(hip, ptr, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    hip._chk(hip.lib.mg_memcpy_d2h(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_uint64(nbytes)))
    return out


def _parse(hip, files, lead):
    """The files back to back behind `lead` bytes of other text (the first file then starts at any alignment) -> what came out."""
    text = b">lead\nACGT\nACGTACGT"[:lead] + b"".join(files) + b"ACGT>\n"  # (what surrounds the files is not theirs)
    ext = np.cumsum([lead] + [len(f) for f in files]).astype(np.uint64)
    d = hip.array(np.frombuffer(text + b"\0" * 32, dtype=np.uint8))
    g = hip.parse_genomes_dev(d.ptr, ext)
    try:
        bases, offs = g.download()
        pb, po = g.device_ptrs()
        guards = (_peek(hip, pb + g.nbases, 16), _peek(hip, po + 8 * (g.count + 1), 8))
        assert g.count == len(files) and g.nbases == int(offs[-1])
        return bytes(bases), [int(o) for o in offs], [int(u) for u in g.undecided], guards
    finally:
        g.free()
        d.free()


def _check(got, want):
    bases, offs, und, guards = got
    assert und == [int(w is None) for w in want]
    assert offs[0] == 0 and all(a <= b for a, b in zip(offs, offs[1:]))
    for f, w in enumerate(want):
        if w is not None:
            assert bases[offs[f]:offs[f + 1]] == w, "file %d" % f
    assert all((g == GUARD).all() for g in guards), "the parser wrote behind its bases / offsets"


# ---- 1. text in HBM -> genomes ----
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_parse_dev_is_genome_bases(hip, knobs, wanted, name):
    knobs("genome_guard", 1)
    for lead in (0, 1 + sorted(gc.CASES).index(name) % 15):
        _check(_parse(hip, gc.CASES[name], lead), wanted[name])


def test_parse_dev_all_cases_in_one_batch(hip, knobs, wanted):
    knobs("genome_guard", 1)
    names = sorted(gc.CASES)
    files = [f for n in names for f in gc.CASES[n]]
    want = [w for n in names for w in wanted[n]]
    got = _parse(hip, files, 5)
    _check(got, want)
    decided = [f for f, w in enumerate(want) if w is not None]
    # offsets included: between decided neighbours a genome is exactly as long as the definition says
    assert all(got[1][f + 1] - got[1][f] == len(want[f]) for f in decided)


def test_parse_dev_no_files(hip):
    g = hip.parse_genomes_dev(0, np.zeros(1, np.uint64))
    assert g.count == 0 and g.nbases == 0
    g.free()


# ---- 2. files on disk -> batches ----
def _genome_text(i, nbases):
    recs = [gc.seq(nbases // 3, 50 + i), b"", gc.seq(nbases - nbases // 3, 90 + i, b"ACGTacgtN")]
    return gc.fasta(recs, width=70, final_newline=i % 2 == 0)


@pytest.fixture(scope="module")
def disk_files(tmp_path_factory):
    """12 files: plain, .gz, a two-member .gz with zero padding behind it, BGZF-style .gz files with their empty EOF member (one of
    them holds nothing else), and one 200 KB genome."""
    d = tmp_path_factory.mktemp("organisms")
    paths = []
    for i in range(12):
        text = _genome_text(i, 200000 if i == 4 else 3000 + 500 * i)
        if i == 7:
            text = b""
        kind = ("plain", "gz", "gz2", "bgzf")[i % 4]
        p = d / ("taxid_%d_genomic.fna%s" % (i, "" if kind == "plain" else ".gz"))
        if kind == "plain":
            p.write_bytes(text)
        elif kind == "gz":
            p.write_bytes(gzip.compress(text, 6))
        elif kind == "gz2":
            cut = len(text) // 2 + 1  # (in the middle of a line)
            p.write_bytes(gzip.compress(text[:cut], 1) + gzip.compress(text[cut:], 9) + b"\0" * 7)
        else:
            p.write_bytes(bamgen.bgzf(text, block=4000 if i != 7 else 65280, eof=True))
        paths.append(str(p))
    want = [bytes(np.asarray(build_db.genome_bases(p), dtype=np.uint8)) for p in paths]
    return paths, want


def test_genome_batches_over_files(hip, knobs, disk_files):
    paths, want = disk_files
    knobs("genome_slab_bytes", 64 << 10)  # the 200 KB genome spans >= 3 slabs (its text is ~203 KB)
    assert len(want[4]) >= 200000 and want[7] == b""
    seen, nbatches = [], 0
    for batch in hip.genome_batches(paths, batch_bases=20000, nthreads=3):
        bases, offs = batch.download()
        assert batch.first_file == len(seen) and not batch.undecided.any()
        for f in range(batch.count):
            seen.append(bytes(bases[int(offs[f]):int(offs[f + 1])]))
        nbatches += 1
        batch.free()
    assert seen == want
    assert nbatches >= 3
    assert hip.genome_stream_stats["text_bytes"] >= sum(len(w) for w in want)


def test_genome_batches_one_batch_and_default_slabs(hip, disk_files):
    paths, want = disk_files
    batches = list(hip.genome_batches(paths))
    assert len(batches) == 1 and batches[0].count == len(paths) and batches[0].first_file == 0
    bases, offs = batches[0].download()
    assert [bytes(bases[int(offs[f]):int(offs[f + 1])]) for f in range(len(paths))] == want
    batches[0].free()
    assert list(hip.genome_batches([])) == []


# ---- 3. the sketchers over a parsed batch ----
@pytest.mark.parametrize("hash_mode", [0, 1])
def test_dev_sketchers_equal_the_host_pointer_calls(hip, hash_mode):
    """k 21 and 60, n = 50, 5 genomes of 2-20 kb with an empty one: plain, prefix, k-mers canonical and forward, array for array."""
    lens = [2000, 0, 20000, 7777, 3001]
    files = [gc.fasta([gc.seq(n // 2, 7 * i, b"ACGTN" if i == 3 else b"ACGT"), gc.seq(n - n // 2, 7 * i + 1)], width=70) if n else b">e\n"
             for i, n in enumerate(lens)]
    ext = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)
    d = hip.array(np.frombuffer(b"".join(files) + b"\0" * 32, dtype=np.uint8))
    g = hip.parse_genomes_dev(d.ptr, ext)
    previous = hip.hash_mode
    hip.set_hash_mode(hash_mode)
    try:
        bases, offs = g.download()
        assert [int(b - a) for a, b in zip(offs, offs[1:])] == [n + 1 if n else 0 for n in lens]  # (two records: one 'N')
        hb = bases if len(bases) else np.zeros(1, np.uint8)
        n = 50
        for k in (21, 60):
            for a, b in zip(hip.sketch_genomes_dev(g, k, n), hip.sketch_genomes(hb, offs, k, n)):
                assert np.array_equal(a, b)
            for sh in ("canonical", "forward"):
                for a, b in zip(hip.sketch_genomes_kmers_dev(g, k, n, sketch_hash=sh), hip.sketch_genomes_kmers(hb, offs, k, n, sketch_hash=sh)):
                    assert np.array_equal(a, b)
        for a, b in zip(hip.sketch_genomes_prefix_dev(g, 60, 21, n), hip.sketch_genomes_prefix(hb, offs, 60, 21, n)):
            assert np.array_equal(a, b)
    finally:
        hip.set_hash_mode(previous)
        g.free()
        d.free()


# ---- 4. the table ----
def _organism_dir(tmp_path, undecided_file=False):
    d = tmp_path / "organisms"
    d.mkdir()
    for i in range(10):
        text = _genome_text(i, 4000 + 900 * i)
        if undecided_file and i == 6:
            text = text.replace(b"\n", b"\r", 3).replace(b"\r", b"\n", 1)  # two lone '\r': text mode ends a line there
            assert gc.undecided(text)
        name = "taxid_%d_genomic.fna" % i
        if i % 3 == 1:
            (d / (name + ".gz")).write_bytes(gzip.compress(text, 6))
        else:
            (d / name).write_bytes(text)
    return str(d)


MODES = {"sketch_per_k": ["-k", "21,31,60"],
         "reference_pipeline": ["-k", "21,31,60", "--reference_pipeline"],
         "cmash_prefix_tables": ["-k", "21,31,60", "--hash_mode", "cmash", "--prefix_tables"]}


def _same_tables(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "meta.json" in names and len(names) > 4
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert (mismatch, errors) == ([], []) and match == names


@pytest.mark.parametrize("mode", sorted(MODES))
def test_build_db_device_ingest_writes_the_host_table(hip, tmp_path, mode):
    src = _organism_dir(tmp_path)
    extra = list(MODES[mode])
    for ingest in ("host", "device"):
        build_db.main([src, str(tmp_path / ingest), "-n", "100", "--ingest", ingest] + extra)
    _same_tables(str(tmp_path / "host"), str(tmp_path / "device"))
    assert hip.genomes_host_parsed == 0


def test_build_db_device_ingest_with_an_undecided_file(hip, tmp_path):
    src = _organism_dir(tmp_path, undecided_file=True)
    for ingest in ("host", "device"):
        build_db.main([src, str(tmp_path / ingest), "-n", "100", "-k", "21,31", "--ingest", ingest])
    _same_tables(str(tmp_path / "host"), str(tmp_path / "device"))
    assert hip.genomes_host_parsed == 1


# ---- 5. files that cannot be read ----
def test_truncated_gz_and_unreadable_path_fail_the_build(hip, tmp_path):
    src = _organism_dir(tmp_path)
    whole = gzip.compress(_genome_text(3, 50000), 6)
    bad = os.path.join(src, "taxid_55_genomic.fna.gz")
    with open(bad, "wb") as fh:
        fh.write(whole[: len(whole) // 2])
    with pytest.raises(_hip.HipError, match="taxid_55_genomic.fna.gz"):
        build_db.main([src, str(tmp_path / "t1"), "-n", "100", "-k", "21", "--ingest", "device"])
    assert not os.path.exists(str(tmp_path / "t1"))
    with open(bad, "wb") as fh:  # whole members, then bytes that are no gzip member
        fh.write(whole + b"not gzip")
    with pytest.raises(_hip.HipError, match="taxid_55_genomic.fna.gz"):
        build_db.main([src, str(tmp_path / "t2"), "-n", "100", "-k", "21", "--ingest", "device"])
    os.remove(bad)
    lst = tmp_path / "list.txt"
    missing = os.path.join(src, "taxid_77_missing.fna")
    lst.write_text("\n".join(sorted(os.path.join(src, f) for f in os.listdir(src)) + [missing]) + "\n")
    with pytest.raises(_hip.HipError, match="taxid_77_missing.fna"):
        build_db.main([str(lst), str(tmp_path / "t3"), "-n", "100", "-k", "21", "--ingest", "device"])
    assert not os.path.exists(str(tmp_path / "t2")) and not os.path.exists(str(tmp_path / "t3"))
    # and the stream is usable afterwards
    build_db.main([src, str(tmp_path / "t4"), "-n", "100", "-k", "21", "--ingest", "device"])
    assert os.path.exists(str(tmp_path / "t4" / "meta.json"))
