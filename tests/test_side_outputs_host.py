"""metalign_amd/side_outputs.py and the driver around it, without a GPU or the library: a stub `hip` stands in for both.

What is held here: every accumulator that was opened is freed exactly once on every way out; the order coverage, depth, identity;
the exits when the device refuses the memory; the memory estimate; the refusals; and which tokeniser entry point
map_and_process_file reaches for every combination of its switches.  The expected figures, strings and calls are written out from
the code as it stood before the side outputs had one protocol."""
import itertools

import pytest

import stage_c_checks as sc
from metalign_amd import _hip, map_and_profile as mp, side_outputs as so

LENGTHS = {"a": 2 ** 23, "b": 2 ** 23}
ACC_INDEX = {"a": 0, "b": 1}
ACC2INFO = {"Unmapped": [0, "Unmapped", "n", "t"], "a": [2 ** 23, "1", "n|a", "t|1"], "b": [2 ** 23, "2", "n|b", "t|2"]}
AB2INFO = {k: v for k, v in ACC2INFO.items() if k != "Unmapped"}  # (the accessions LENGTHS and ACC_INDEX know)
TAXID2INFO = {"Unmapped": [0, "strain", "n", "t"], "1": [2 ** 23, "strain", "n|a", "t|1"], "2": [2 ** 23, "strain", "n|b", "t|2"]}


class Boom(Exception):
    pass


class FakeAcc:
    """A recording accumulator: fail = the step at which it raises Boom."""

    def __init__(self, name, log, fail=None, window=0):
        self.name, self.log, self.fail, self.window, self.frees = name, log, fail, window, 0

    def _step(self, what):
        self.log.append((what, self.name))
        if self.fail == what:
            raise Boom(what + " " + self.name)

    def add_batch(self, batch, pct_id):
        self._step("add")

    def add_ptr(self, d_recs, d_side, n, pct_id):
        self.log.append(("side", self.name, d_side))
        self._step("add")

    def result(self):
        self._step("close")
        zeros = [0, 0]
        return {"coverage": (zeros, zeros, zeros, 0), "depth": (zeros, 0, {}, {}), "identity": (zeros, zeros, zeros, 0, {})}[self.name]

    def free(self):
        self.frees += 1


class StubHip:
    """coverage / depth / identity hand out FakeAccs; fail = {family name: step}, 'open' among the steps."""

    def __init__(self, fail=None):
        self.log, self.made, self.fail = [], [], dict(fail or {})

    def _make(self, name, window=0):
        self.log.append(("open", name))
        if self.fail.get(name) == "open":
            raise Boom("open " + name)
        if isinstance(self.fail.get(name), _hip.HipError):
            raise self.fail[name]
        self.made.append(FakeAcc(name, self.log, self.fail.get(name), window))
        return self.made[-1]

    def coverage(self, lengths):
        return self._make("coverage")

    def depth(self, lengths, window=0):
        return self._make("depth", window)

    def identity(self, nacc):
        return self._make("identity")


def _args(tmp_path, **extra):
    return sc.make_args(str(tmp_path / "x.sam"), str(tmp_path / "db_info.txt"), str(tmp_path / "o.cami"), extra)


def _all_on(tmp_path, **extra):
    return _args(tmp_path, coverage=str(tmp_path / "c.tsv"), depth=str(tmp_path / "d.tsv"), depth_windows=str(tmp_path / "w.tsv"),
                 depth_window_size=1000, identity=str(tmp_path / "i.tsv"), **extra)


def _cycle(sides, hip, by_ptr):
    sides.open(hip, LENGTHS, ACC_INDEX)
    if by_ptr:
        sides.add_ptrs(1, 2, 3, 5, 0.5)
    else:
        sides.add_batch(object(), 0.5)
    sides.close(AB2INFO, TAXID2INFO)


# ---- cleanup and order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_ptr", [False, True])
def test_success_frees_each_once_in_the_order_coverage_depth_identity(tmp_path, by_ptr):
    args = _all_on(tmp_path)
    so.write_headers(args)
    hip = StubHip()
    sides = so.SideOutputs.of(args, "x.sam")
    assert sides and sides.placed and sides.edited
    _cycle(sides, hip, by_ptr)
    order = ["coverage", "depth", "identity"]
    for step in ("open", "add", "close"):
        assert [n for s, n in [e[:2] for e in hip.log] if s == step] == order
    assert [f.frees for f in hip.made] == [1, 1, 1]
    if by_ptr:  # coverage and depth read the places, identity the edits
        assert [e[1:] for e in hip.log if e[0] == "side"] == [("coverage", 2), ("depth", 2), ("identity", 3)]
    sides.free()
    assert [f.frees for f in hip.made] == [1, 1, 1]
    for name in ("c.tsv", "d.tsv", "i.tsv"):  # a header and a block each (no window is kept: w.tsv holds its header alone)
        assert (tmp_path / name).read_text().count("\n") >= 2


@pytest.mark.parametrize("by_ptr", [False, True])
@pytest.mark.parametrize("family, step, opened", [("depth", "open", 1), ("identity", "open", 2), ("coverage", "add", 3),
                                                  ("depth", "add", 3), ("coverage", "close", 3), ("depth", "close", 3)])
def test_a_failure_frees_what_was_opened_once_and_propagates(tmp_path, family, step, opened, by_ptr):
    args = _all_on(tmp_path)
    so.write_headers(args)
    hip = StubHip({family: step})
    sides = so.SideOutputs.of(args, "x.sam")
    with pytest.raises(Boom) as e:
        _cycle(sides, hip, by_ptr)
    assert str(e.value) == "%s %s" % (step, family)
    assert len(hip.made) == opened and [f.frees for f in hip.made] == [1] * opened
    sides.free()  # (what a caller's own handler does on top)
    assert [f.frees for f in hip.made] == [1] * opened


def test_only_what_was_asked_for_is_opened(tmp_path):
    hip = StubHip()
    sides = so.SideOutputs.of(_args(tmp_path, identity=str(tmp_path / "i.tsv")), "x.sam")
    assert sides and sides.edited and not sides.placed
    sides.open(hip, None, ACC_INDEX)
    sides.free()
    assert hip.log == [("open", "identity")] and hip.made[0].frees == 1
    assert not so.SideOutputs.of(_args(tmp_path), "x.sam")
    assert not so.SideOutputs.of(_all_on(tmp_path), "x.sam", enabled=False)
    assert not so.SideOutputs.of(_args(tmp_path, coverage=None, depth="NONE"), "x.sam")


def test_source_label_only_with_more_than_one_input(tmp_path):
    args = _args(tmp_path)
    assert so.source_label(args, "x.sam") is None
    args.infiles = ["x.sam", "y.sam"]
    assert so.source_label(args, "y.sam") == "y.sam"
    del args.infiles
    assert so.source_label(args, "y.sam") is None


# ---- ERR_NOMEM ----------------------------------------------------------------------------------------------------------------
def test_nomem_exits_with_the_three_messages(tmp_path):
    args = _all_on(tmp_path)
    total, nacc, window = 2 ** 23 + 2 ** 23, 2, 1000
    nwin = 2 * ((2 ** 23 + window - 1) // window)
    want = {
        "coverage": "Error: --coverage keeps one bit per reference base on the GPU; %d MB for this database do not fit." % (total >> 23),
        "depth": "Error: --depth keeps four bytes per reference base on the GPU; %d MB for this database do not fit."
                 % ((4 * (total + nacc) + 12 * nwin + 8 * 4096 * min(nacc, 0)) >> 20),
        "identity": "Error: --identity keeps 1001 bins of eight bytes per accession on the GPU; %d MB for this database do not fit."
                    % ((8 * (1001 + 3) * nacc + 16 * 0) >> 20),
    }
    assert want["coverage"].count(" 2 MB") and want["depth"].count(" 64 MB") and want["identity"].count(" 0 MB")
    for name, text in want.items():
        hip = StubHip({name: _hip.HipError("x", _hip.ERR_NOMEM)})
        sides = so.SideOutputs.of(args, "x.sam")
        with pytest.raises(SystemExit) as e:
            sides.open(hip, LENGTHS, ACC_INDEX)
        assert e.value.code == text
        assert all(f.frees == 1 for f in hip.made)
        other = _hip.HipError("y", _hip.ERR_ARG)
        hip = StubHip({name: other})
        with pytest.raises(_hip.HipError) as e:
            so.SideOutputs.of(args, "x.sam").open(hip, LENGTHS, ACC_INDEX)
        assert e.value is other and all(f.frees == 1 for f in hip.made)


# ---- the memory estimate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrec", [0, 1000])
@pytest.mark.parametrize("window", [0, 1000, 7])
@pytest.mark.parametrize("cov, dep, idn", list(itertools.product([False, True], repeat=3)))
def test_need_bytes_is_the_former_arithmetic(tmp_path, cov, dep, idn, window, nrec):
    lengths = {"a": 2 ** 23, "b": 12345, "c": 0}
    nacc = len(lengths)
    extra = {}
    if cov:
        extra["coverage"] = "c.tsv"
    if dep:
        extra.update({"depth_windows": "w.tsv", "depth_window_size": window} if window else {"depth": "d.tsv"})
    if idn:
        extra["identity"] = "i.tsv"
    need = 0
    if cov or dep:
        need += 16 * nrec
        if cov:
            need += sum(lengths.values()) // 8
        if dep:
            nwin = sum((n + window - 1) // window for n in lengths.values()) if window else 0
            need += 4 * (sum(lengths.values()) + len(lengths)) + 12 * nwin + 8 * 4096 * min(len(lengths), nrec)
    if idn:
        need += 8 * (1001 + 3) * nacc + 16 * nrec
    sides = so.SideOutputs.of(_args(tmp_path, **extra), "x.sam")
    assert sides.need_bytes(lengths if sides.placed else None, nacc, nrec) == need
    assert (sides.placed, sides.edited) == (cov or dep, idn)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
WORLD = {
    "read_assignments": "Error: --read_assignments runs in one process on one GPU; start it without torch.distributed.run.",
    "coverage": "Error: --coverage runs in one process on one GPU; start it without torch.distributed.run.",
    "depth": "Error: --depth and --depth_windows run in one process on one GPU; start it without torch.distributed.run.",
    "depth_windows": "Error: --depth and --depth_windows run in one process on one GPU; start it without torch.distributed.run.",
    "identity": "Error: --identity runs in one process on one GPU; start it without torch.distributed.run.",
}
PAF = {
    "coverage": "Error: --coverage needs SAM or BAM alignments: a PAF line has no POS and CIGAR columns.",
    "depth": "Error: --depth and --depth_windows need SAM or BAM alignments: a PAF line has no POS and CIGAR columns.",
    "depth_windows": "Error: --depth and --depth_windows need SAM or BAM alignments: a PAF line has no POS and CIGAR columns.",
    "identity": "Error: --identity needs SAM or BAM alignments: the NM:i: and cg:Z: tags of a PAF line are not read.",
}


def _never(*a, **k):
    raise AssertionError("refused before the process group, the GPU or the library is touched")


@pytest.fixture
def untouchable(monkeypatch):
    from metalign_amd import select_db
    monkeypatch.setattr(_hip.Hip, "get", _never)
    monkeypatch.setattr(_hip, "load_library", _never)
    monkeypatch.setattr(select_db, "dist_context", _never)
    monkeypatch.setattr(select_db, "select_main", _never)
    monkeypatch.setattr(mp, "get_acc2info", _never)


def _refused(fn, *a):
    with pytest.raises(SystemExit) as e:
        fn(*a)
    return e.value.code


@pytest.mark.parametrize("flag", sorted(WORLD))
def test_every_family_is_refused_under_two_processes(untouchable, monkeypatch, tmp_path, flag):
    from metalign_amd import metalign
    monkeypatch.setenv("WORLD_SIZE", "2")
    out = tmp_path / "out.tsv"
    assert _refused(mp.map_main, _args(tmp_path, **{flag: str(out)})) == WORLD[flag]
    assert _refused(metalign.main, ["r.fq", "data", "--" + flag, str(out)]) == WORLD[flag]
    assert not out.exists()


@pytest.mark.parametrize("flag", sorted(PAF))
def test_every_family_is_refused_on_a_paf_input(untouchable, tmp_path, flag):
    out = tmp_path / "out.tsv"
    args = _args(tmp_path, **{flag: str(out), "input_type": "AUTO"})
    args.infiles = [str(tmp_path / "x.paf")]
    assert _refused(mp.map_main, args) == PAF[flag]
    assert _refused(mp.map_main, _args(tmp_path, **{flag: str(out), "paf_input": True})) == PAF[flag]
    assert not out.exists()


def test_the_order_of_the_refusals(untouchable, monkeypatch, tmp_path):
    everything = dict(read_assignments="r.tsv", coverage="c.tsv", depth="d.tsv", identity="i.tsv", depth_window_size=0, paf_input=True,
                      multimap_iterations=0)
    order = [("coverage", PAF["coverage"]), ("depth", PAF["depth"]), ("identity", PAF["identity"]),
             ("depth_window_size", "Error: --depth_window_size must be at least 1."),
             ("multimap_iterations", "Error: --multimap_iterations must be at least 1.")]
    for drop, text in order:
        assert _refused(mp.map_main, _args(tmp_path, **everything)) == text
        del everything[drop]
    monkeypatch.setenv("WORLD_SIZE", "2")
    everything = dict(read_assignments="r.tsv", coverage="c.tsv", depth="d.tsv", identity="i.tsv", paf_input=True)
    for drop in ("read_assignments", "coverage", "depth", "identity"):
        assert _refused(mp.map_main, _args(tmp_path, **everything)) == WORLD[drop]
        del everything[drop]


# ---- which tokeniser entry point map_and_process_file reaches -----------------------------------------------------------------
class Stop(Exception):
    pass


class _Freeable:
    ptr = count = places_ptr = edits_ptr = 0

    def __init__(self):
        self.frees = 0

    def free(self):
        self.frees += 1


class DispatchHip(StubHip):
    """Records the tokeniser call (every keyword, the defaults of metalign_amd._hip.Hip filled in) and stops at stage C."""

    def __init__(self):
        super().__init__()
        self.calls, self.batch, self.index, self.text = [], _Freeable(), _Freeable(), _Freeable()

    def mem_info(self):
        return 1 << 50, 1 << 50, 0

    def acc_index(self, names):
        assert names == ["Unmapped", "a", "b"]
        return self.index

    def upload_file(self, path):
        self.calls.append(("upload_file", path))
        return self.text, 4242

    def sam_tokenize_dev_batch(self, d_text, nbytes, acc_index, prev_qname="", paf=False, named=False, placed=False, keyed=False,
                               collate=False, edited=False):
        assert (d_text, nbytes, acc_index, prev_qname) == (self.text.ptr, 4242, self.index, "")
        self.calls.append(("sam_tokenize_dev_batch", dict(paf=paf, named=named, placed=placed, keyed=keyed, collate=collate, edited=edited)))
        return self.batch

    def sam_stream_file(self, path, acc_index, paf=False, offset=0, length=0, chunk_bytes=0, nthreads=0, collate=False, named=False,
                        placed=False, edited=False):
        assert acc_index is self.index
        self.calls.append(("sam_stream_file", path, dict(paf=paf, offset=offset, length=length, chunk_bytes=chunk_bytes, nthreads=nthreads,
                                                         collate=collate, named=named, placed=placed, edited=edited)))
        return self.batch

    def bam_stream_file(self, path, acc_index, chunk_bytes=0, nthreads=0, collate=False, named=False, placed=False, edited=False):
        assert acc_index is self.index
        self.calls.append(("bam_stream_file", path, dict(chunk_bytes=chunk_bytes, nthreads=nthreads, collate=collate, named=named,
                                                         placed=placed, edited=edited)))
        return self.batch

    def profile_assign_dev_records(self, ptr, count, ref2tax, ntax, pct_id, owners, resident=False, assign=False):
        self.calls.append(("stage C", dict(resident=resident, assign=assign)))
        raise Stop()


def _former_dispatch(path, sided, streamed, _bam, _collate, _paf, _assignments, placed, edited, chunk):
    """The six branches as they stood, with the keywords each of them wrote (what it left out: the method's default)."""
    tok = dict(paf=False, named=False, placed=False, keyed=False, collate=False, edited=False)
    sam = dict(paf=False, offset=0, length=0, chunk_bytes=0, nthreads=0, collate=False, named=False, placed=False, edited=False)
    bam = dict(chunk_bytes=0, nthreads=0, collate=False, named=False, placed=False, edited=False)
    if sided and not streamed and not _bam and not _collate:
        return [("upload_file", path), ("sam_tokenize_dev_batch", dict(tok, named=_assignments, placed=placed, edited=edited))]
    if sided:
        if _bam:
            return [("bam_stream_file", path, dict(bam, chunk_bytes=chunk, collate=_collate, named=_assignments, placed=placed, edited=edited))]
        return [("sam_stream_file", path, dict(sam, chunk_bytes=chunk, collate=_collate, named=_assignments, placed=placed, edited=edited))]
    if _bam:
        return [("bam_stream_file", path, dict(bam, chunk_bytes=chunk, collate=_collate, named=_assignments))]
    if _collate:
        return [("sam_stream_file", path, dict(sam, paf=_paf, chunk_bytes=chunk, collate=True))]
    if not streamed:
        return [("upload_file", path), ("sam_tokenize_dev_batch", dict(tok, paf=_paf, named=_assignments))]
    return [("sam_stream_file", path, dict(sam, paf=_paf, chunk_bytes=chunk, named=_assignments))]


def _dispatch_cases():
    for _bam, _collate, _assignments, placed, edited, no_stream, gz, _paf in itertools.product([False, True], repeat=8):
        if _assignments and _collate:
            continue  # (a named batch is not collated)
        if _paf and (_bam or placed or edited):
            continue  # (a PAF replay is SAM text without side outputs: check_flags refuses the rest)
        yield _bam, _collate, _assignments, placed, edited, no_stream, gz, _paf


@pytest.mark.parametrize("_bam, _collate, _assignments, placed, edited, no_stream, gz, _paf", list(_dispatch_cases()))
def test_dispatch_reaches_the_former_entry_point(monkeypatch, tmp_path, _bam, _collate, _assignments, placed, edited, no_stream, gz, _paf):
    path = str(tmp_path / "in.sam")
    with open(path, "wb") as fh:
        fh.write((b"\x1f\x8b" if gz else b"@H") + b"x" * 1000)
    monkeypatch.setenv("MG_STREAM_CHUNK_BYTES", "65536")
    if no_stream:
        monkeypatch.setenv("MG_NO_STREAM", "1")
    else:
        monkeypatch.delenv("MG_NO_STREAM", raising=False)
    hip = DispatchHip()
    monkeypatch.setattr(_hip.Hip, "get", classmethod(lambda cls, *a, **k: hip))
    args = _all_on(tmp_path)
    sides = so.SideOutputs(args, ([so.COVERAGE] if placed else []) + ([so.IDENTITY] if edited else []), path, header=[])
    with pytest.raises(Stop):
        mp.map_and_process_file(args, path, ACC2INFO, TAXID2INFO, _paf=_paf, _bam=_bam, _collate=_collate, _assignments=_assignments,
                                _sides=sides)
    sided = placed or edited
    streamed = not no_stream or (sided and gz)  # (a gzip file with side arrays is streamed even under MG_NO_STREAM=1)
    want = _former_dispatch(path, sided, streamed, _bam, _collate, _paf, _assignments, placed, edited, 65536)
    assert hip.calls == want + [("stage C", dict(resident=False, assign=_assignments))]
    assert [e for e in hip.log if e[0] in ("open", "add")] == [(s, n) for s in ("open", "add") for n in
                                                                (["coverage"] if placed else []) + (["identity"] if edited else [])]
    # stage C failed: the accumulators, the batch, the index and the text are each freed once
    assert all(f.frees == 1 for f in hip.made)
    assert hip.batch.frees == 1 and hip.index.frees == 1 and hip.text.frees == (1 if want[0][0] == "upload_file" else 0)


def test_the_keywords_of_map_and_process_become_the_object(monkeypatch, tmp_path):
    """_coverage=, _depth=, _identity= (the name the block is written under) reach the streaming path as one SideOutputs."""
    seen = []
    hip = DispatchHip()
    hip.array = lambda host: _Freeable()
    monkeypatch.setattr(_hip.Hip, "get", classmethod(lambda cls, *a, **k: hip))
    monkeypatch.setattr(mp, "_device_tokenise", lambda instream, acc_index, decode=False, collect=None: None)
    monkeypatch.setattr(mp, "_stage_c", lambda args, batch, sides, *a: seen.append(sides) or "done")
    args = _all_on(tmp_path)
    assert mp.map_and_process(args, [], ACC2INFO, TAXID2INFO, _depth="f.sam", _identity="f.sam") == "done"
    assert seen[0].families == (so.DEPTH, so.IDENTITY) and seen[0].source == "f.sam" and seen[0].placed and seen[0].edited
    assert mp.map_and_process(args, [], ACC2INFO, TAXID2INFO, _coverage="g.sam") == "done"
    assert seen[1].families == (so.COVERAGE,) and seen[1].source == "g.sam" and not seen[1].edited
    with pytest.raises(ValueError, match="need the device path"):
        mp.map_and_process(args, [], ACC2INFO, TAXID2INFO, _coverage="g.sam", _assign=lambda *a: None)
