"""The one body behind stage C's entry points (map_and_profile._stage_c), its two carriers (a SamBatch, _hip.UploadedBatch) and the
chunked tokeniser's collector (map_and_profile.TokenisedChunks), without a GPU or the library: a stub `hip` stands in for both.

What is held here: the sequence open / add / stage C / on_verdicts / close that the rule "the accumulators are closed as soon as they
have been fed" gives, the same for both carriers; every device object freed exactly once whatever step fails; the empty stream; and the
collector's join against arrays written out by hand."""
import itertools

import numpy as np
import pytest

import stage_c_checks as sc
from metalign_amd import _hip, coverage, map_and_profile as mp, side_outputs as so

ACC2INFO = {"Unmapped": [0, "Unmapped", "n", "t"], "a": [2 ** 23, "1", "n|a", "t|1"], "b": [2 ** 23, "2", "n|b", "t|2"]}
TAXID2INFO = {"Unmapped": [0, "strain", "n", "t"], "1": [2 ** 23, "strain", "n|a", "t|1"], "2": [2 ** 23, "strain", "n|b", "t|2"]}
FAMILIES = ["coverage", "depth", "identity", "variants"]
SIDE_OF = {"coverage": "places", "depth": "places", "identity": "edits", "variants": ("bases", "pool")}
NREC = 5


class Boom(Exception):
    pass


class Arr:
    """What hip.array / hip.empty hand out: free() as DeviceArray's, the frees that reach the device counted."""
    at = 1000

    def __init__(self):
        Arr.at += 16
        self.ptr, self.frees = Arr.at, 0

    def free(self):
        if self.ptr:
            self.ptr, self.frees = None, self.frees + 1


class Acc:
    """A recording accumulator whose add_batch is the library binding's own (nothing is added for an empty batch)."""

    def __init__(self, hip, name):
        self.hip, self.name, self.frees, self.window = hip, name, 0, 0
        self._side_ptr = {"coverage": "places_ptr", "depth": "places_ptr", "identity": "edits_ptr"}.get(name)

    def add_batch(self, batch, pct_id):
        (_hip.VariantsAcc if self.name == "variants" else _hip._SideAccumulator).add_batch(self, batch, pct_id)

    def add_ptr(self, d_recs, d_side, n, pct_id):
        self.hip.step("add", self.name, d_recs, d_side, n)

    def result(self, *params):
        self.hip.step("close", self.name)
        z = [0, 0, 0]
        return {"coverage": (z, z, z, 0), "depth": (z, 0, {}, {}), "identity": (z, z, z, 0, {}), "variants": (z, z, z, z, z, 0, [])}[self.name]

    def free(self):
        self.frees += 1


class Hip:
    """fail: the step — ('open', family), ('upload', k-th array), ('add', family), ('stage C',), ('on_verdicts',), ('close', family) — at
    which Boom is raised.  Stage C keeps to the binding's ownership: it frees its owners when it returns without `resident`, hands
    them to the ResidentProfile with it, and leaves them alone when it fails."""

    def __init__(self, fail=None):
        self.log, self.accs, self.arrays, self.fail = [], [], [], fail

    def step(self, *what):
        self.log.append(what)
        if self.fail == what[:len(self.fail or ())]:
            raise Boom(what)

    def _open(self, name):
        self.step("open", name)
        self.accs.append(Acc(self, name))
        return self.accs[-1]

    coverage = lambda self, lengths: self._open("coverage")
    depth = lambda self, lengths, window=0: self._open("depth")
    identity = lambda self, nacc: self._open("identity")
    variants = lambda self, lengths: self._open("variants")

    def array(self, host, dtype=None):
        self.step("upload", len(self.arrays))
        self.arrays.append(Arr())
        return self.arrays[-1]

    def empty(self, count, dtype):
        self.arrays.append(Arr())
        self.copy = self.arrays[-1].ptr
        return self.arrays[-1]

    def sync(self):
        pass

    def records_mask_unique(self, d_recs, n, d_words, nreads, d_ref2tax, nref, d_out):
        self.step("on_verdicts", d_recs, n, d_out)

    def profile_assign_dev_records(self, ptr, n, ref2tax, ntax, pct_id, owners, resident=False, assign=False, on_verdicts=None):
        self.step("stage C", ptr, n, dict(resident=resident, assign=assign, hooked=on_verdicts is not None))
        if on_verdicts is not None:
            on_verdicts(ptr, n, 71, 2, 72, len(ref2tax))
        z = np.zeros(ntax, dtype=np.uint64)
        res = dict(count=z, bases=z, first_seen=z, tot_rds=1, n_ambig=0, mm_offsets=np.zeros(1, np.uint64), mm_tax=np.zeros(0, np.uint32),
                   mm_hitlen=np.zeros(0, np.uint64))
        if assign:
            res.update(assign=np.zeros(0, np.uint64), names=owners[0].names())
        if resident:
            res.update(mm_nreads=0, resident=_hip.ResidentProfile(Arr(), list(owners)))
        else:
            for o in owners:
                o.free()
        return res


class StubSamBatch:
    """The surface of a SamBatch that stage C reads; free() as SamBatch's."""

    def __init__(self, n):
        self.ptr, self.count, self.places_ptr, self.edits_ptr, self.bases_ptr, self.pool_ptr = 11, n, 12, 13, 14, 15
        self.handle, self.frees = True, 0

    def names(self):
        return b"", np.zeros(1, dtype=np.uint64)

    def free(self):
        if self.handle:
            self.handle, self.frees = None, self.frees + 1


def _uploaded(hip, n):
    return _hip.UploadedBatch(hip, np.zeros(n, _hip.REC_DTYPE), places=np.zeros(n, _hip.PLACE_DTYPE), edits=np.zeros(n, _hip.EDIT_DTYPE),
                              bases=(np.zeros(n, _hip.BASES_DTYPE), b""), names=(b"", np.zeros(1, dtype=np.uint64)))


CARRIERS = {"SamBatch": lambda hip, n: StubSamBatch(n), "UploadedBatch": _uploaded}


def _args(tmp_path, mode):
    t = lambda name: str(tmp_path / name)
    return sc.make_args(t("x.sam"), t("db_info.txt"), t("o.cami"), dict(
        coverage=t("c.tsv"), depth=t("d.tsv"), identity=t("i.tsv"), variants=t("v.tsv"), read_assignments=t("r.tsv"), side_reads=mode))


def _drive(monkeypatch, tmp_path, hip, carrier, mode, n=NREC, assignments=False, resident=False, sided=True):
    """-> (the batch, the SideOutputs, the roles of the batch's pointers, what _stage_c returned or the exception it raised)."""
    monkeypatch.setattr(_hip.Hip, "get", classmethod(lambda cls, *a, **k: hip))
    args = _args(tmp_path, mode)
    sides = so.SideOutputs.of(args, "x.sam", enabled=sided)
    batch = CARRIERS[carrier](hip, n)
    role = {batch.ptr: "recs"}
    if n or carrier == "SamBatch":
        role.update({batch.places_ptr: "places", batch.edits_ptr: "edits", batch.bases_ptr: "bases", batch.pool_ptr: "pool"})
    del hip.log[:]  # (the carrier's own uploads are not the driver's)
    tables = mp.dense_tables(ACC2INFO, TAXID2INFO)
    try:
        out = mp._stage_c(args, batch, sides, coverage.lengths_of([], ACC2INFO), tables, ACC2INFO, TAXID2INFO, resident, assignments, False)
    except Boom as e:
        out = e
    role[getattr(hip, "copy", None)] = "copy"
    return batch, sides, role, out


def _named(log, role):
    """The log with the batch's pointers by their roles."""
    name = lambda x: tuple(name(y) for y in x) if isinstance(x, tuple) else role.get(x, x) if isinstance(x, int) and x > 10 else x
    return [tuple(name(x) for x in e) for e in log]


def _expected(mode, n, assignments, resident):
    """What the rule gives: under `all` the accumulators are fed and closed before stage C; under `unique` stage C feeds them the masked
    copy of the records through its hook and they are closed directly after it.  Nothing is added for an empty stream."""
    opens = [("open", f) for f in FAMILIES]
    closes = [("close", f) for f in FAMILIES]
    adds = [("add", f, "copy" if mode == "unique" else "recs", SIDE_OF[f], n) for f in FAMILIES] if n else []
    stage_c = [("stage C", "recs", n, dict(resident=resident, assign=assignments, hooked=mode == "unique"))]
    if mode == "all":
        return opens + adds + closes + stage_c
    return opens + stage_c + ([("on_verdicts", "recs", n, "copy")] if n else []) + adds + closes


# ---- 1. the driver's sequence of calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, assignments, resident", list(itertools.product(["all", "unique"], [False, True], [False, True])))
def test_the_sequence_is_the_rules_and_the_same_for_both_carriers(monkeypatch, tmp_path, mode, assignments, resident):
    logs = {}
    for carrier in CARRIERS:
        hip = Hip()
        batch, sides, role, out = _drive(monkeypatch, tmp_path, hip, carrier, mode, assignments=assignments, resident=resident)
        taxids2abs, mm, low = out
        assert list(taxids2abs) == ["Unmapped"] and low == {} and mm["taxids"] == list(TAXID2INFO)
        logs[carrier] = _named(hip.log, role)
        assert logs[carrier] == _expected(mode, NREC, assignments, resident)
        assert [a.frees for a in hip.accs] == [1] * 4
        if resident:  # (the batch lives on with the resident profile, whose owner frees it)
            assert batch.count == NREC and _frees_of(hip, batch, carrier) == 0
            mm["resident"].free()
        assert _frees_of(hip, batch, carrier) == 1
        assert all(a.frees == 1 for a in hip.arrays)
    assert logs["SamBatch"] == logs["UploadedBatch"]


def _frees_of(hip, batch, carrier):
    """How often the batch's device memory was freed (an UploadedBatch's: every array of it as often)."""
    if carrier == "SamBatch":
        return batch.frees
    mine = [a.frees for a in hip.arrays[:5 if batch.count else 1]]
    assert len(set(mine)) == 1
    return mine[0]


def test_without_side_outputs_it_is_stage_c_alone(monkeypatch, tmp_path):
    """The ranks' gathered records: a carrier without side arrays and an empty SideOutputs."""
    hip = Hip()
    monkeypatch.setattr(_hip.Hip, "get", classmethod(lambda cls, *a, **k: hip))
    batch = _hip.UploadedBatch(hip, np.zeros(8, np.int32).view(_hip.REC_DTYPE))
    assert batch.count == 2
    for side in ("places_ptr", "edits_ptr", "bases_ptr", "pool_ptr", "names"):
        with pytest.raises(_hip.HipError) as e:
            getattr(batch, side)() if side == "names" else getattr(batch, side)
        assert e.value.code == _hip.ERR_STATE
    args = _args(tmp_path, "all")
    mp._stage_c(args, batch, so.SideOutputs(args, (), "x.sam"), None, mp.dense_tables(ACC2INFO, TAXID2INFO), ACC2INFO, TAXID2INFO)
    assert hip.log[1:] == [("stage C", batch.ptr, 2, dict(resident=False, assign=False, hooked=False))]
    assert [a.frees for a in hip.arrays] == [1]


# ---- 2. every device object is freed exactly once -------------------------------------------------------------------------------
FAILURES = ([("open", f) for f in FAMILIES] + [("add", f) for f in FAMILIES] + [("stage C",), ("on_verdicts",)]
            + [("close", f) for f in FAMILIES])


@pytest.mark.parametrize("carrier", list(CARRIERS))
@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("fail, mode", [(f, m) for f in FAILURES for m in ("all", "unique") if (f, m) != (("on_verdicts",), "all")],
                         ids=lambda x: " ".join(x) if isinstance(x, tuple) else x)  # (there is no hook under --side_reads all)
def test_a_failure_at_any_step_frees_everything_once_and_propagates(monkeypatch, tmp_path, fail, mode, resident, carrier):
    hip = Hip(fail)
    batch, sides, role, out = _drive(monkeypatch, tmp_path, hip, carrier, mode, assignments=True, resident=resident)
    assert isinstance(out, Boom) and out.args[0][:len(fail)] == fail
    opened = FAMILIES.index(fail[1]) if fail[0] == "open" else 4
    assert len(hip.accs) == opened and [a.frees for a in hip.accs] == [1] * opened
    assert _frees_of(hip, batch, carrier) == 1 and all(a.frees == 1 for a in hip.arrays)
    batch.free()  # (what a caller's own handler does on top)
    sides.free()
    assert _frees_of(hip, batch, carrier) == 1 and all(a.frees == 1 for a in hip.arrays) and [a.frees for a in hip.accs] == [1] * opened


@pytest.mark.parametrize("k", range(5))
def test_a_failing_upload_frees_what_was_uploaded_before_it(k):
    """The records, the places, the edits, the entries, the pool: the k-th of them fails inside UploadedBatch's construction."""
    hip = Hip(("upload", k))
    with pytest.raises(Boom) as e:
        _uploaded(hip, NREC)
    assert e.value.args[0] == ("upload", k)
    assert len(hip.arrays) == k and [a.frees for a in hip.arrays] == [1] * k


def test_free_is_idempotent_and_the_pointers_are_the_arrays():
    hip = Hip()
    batch = _uploaded(hip, NREC)
    assert [batch.ptr, batch.places_ptr, batch.edits_ptr, batch.bases_ptr, batch.pool_ptr] == [a.ptr for a in hip.arrays]
    batch.free()
    batch.free()
    assert [a.frees for a in hip.arrays] == [1] * 5


# ---- 3. zero records --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carrier", list(CARRIERS))
@pytest.mark.parametrize("mode", ["all", "unique"])
def test_an_empty_stream_adds_nothing_runs_stage_c_and_writes_its_blocks(monkeypatch, tmp_path, mode, carrier):
    """As before the one body, on both paths: map_and_process_file fed a batch of count 0 to accumulators whose add_batch skips it, and
    the streaming path put `if len(recs)` around its side uploads and its add; both called stage C with n = 0 and closed the
    accumulators, which appends a block of no rows (checked by running the former two bodies over these stubs)."""
    so.write_headers(_args(tmp_path, mode))
    heads = {f: (tmp_path / f).read_text() for f in ("c.tsv", "d.tsv", "i.tsv", "v.tsv")}
    hip = Hip()
    batch, sides, role, out = _drive(monkeypatch, tmp_path, hip, carrier, mode, n=0)
    assert not isinstance(out, Exception)
    assert _named(hip.log, role) == _expected(mode, 0, False, False)
    assert not [e for e in hip.log if e[0] in ("add", "upload", "on_verdicts")]
    assert len(hip.arrays) == (1 if carrier == "UploadedBatch" else 0)  # (the one zero record a handle needs)
    assert batch.count == 0 and (carrier == "SamBatch" or [batch.places_ptr, batch.edits_ptr, batch.bases_ptr, batch.pool_ptr] == [0] * 4)
    for f, head in heads.items():
        text = (tmp_path / f).read_text()
        assert text.startswith(head) and len(text) > len(head), f
    assert [a.frees for a in hip.accs] == [1] * 4 and _frees_of(hip, batch, carrier) == 1


# ---- 4. the collector's join ----------------------------------------------------------------------------------------------------
def _chunk(nrec, first_ref, names, pool, spans):
    """One chunk's (records, [names, places, edits, bases]) — the entries' offsets run through the chunk's own pool."""
    recs = np.zeros(nrec, dtype=_hip.REC_DTYPE)
    recs[recs.dtype.names[0]] = np.arange(first_ref, first_ref + nrec)
    places = np.array([(first_ref + i, 10 + i) for i in range(nrec)], dtype=_hip.PLACE_DTYPE)
    edits = np.array([(i, first_ref + i) for i in range(nrec)], dtype=_hip.EDIT_DTYPE)
    ent, at = [], 0
    for i, span in enumerate(spans):
        ent.append((at, first_ref + i, span))
        at += (span + 1) // 2
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    return recs, [(b"".join(names), off), places, edits, (np.array(ent, dtype=_hip.BASES_DTYPE), pool)]


CHUNKS = [_chunk(3, 0, [b"r1", b"read2"], b"\x12\x34\x56", [3, 0, 2]),  # (span 0: not piled — its offset, 2, is left as it is)
          _chunk(2, 3, [b"q"], b"", [0, 0]),                            # (nothing piled: an empty pool)
          _chunk(2, 5, [], b"\xab\xcd", [2, 1])]                        # (both records go on with the read before: no name)


@pytest.mark.parametrize("nchunks", [2, 3])
def test_the_join_is_the_former_joiners(nchunks):
    col = mp.TokenisedChunks(named=True, placed=True, edited=True, based=True)
    assert col.want == dict(named=True, placed=True, edited=True, based=True)
    for recs, sides in CHUNKS[:nchunks]:
        col.add(recs, sides)
    got = col.joined()
    assert sorted(got) == ["bases", "edits", "names", "places", "recs"]
    n = [3, 5, 7][nchunks - 1]
    assert got["recs"][got["recs"].dtype.names[0]].tolist() == list(range(n)) and np.array_equal(got["recs"], col.records())
    assert got["places"].tolist() == [(i, 10 + j) for i, j in zip(range(n), [0, 1, 2, 0, 1, 0, 1])]
    assert got["edits"].tolist() == [(j, i) for i, j in zip(range(n), [0, 1, 2, 0, 1, 0, 1])]
    blob, off = got["names"]
    assert blob == b"r1read2q" and off.dtype == np.uint64 and off.tolist() == [0, 2, 7, 8]
    ent, pool = got["bases"]
    # off: the first chunk's as they are; the second's not piled, so NOT moved up by the 3 bytes before them; the third's moved up by 3 + 0
    want = [(0, 0, 3), (2, 1, 0), (2, 2, 2), (0, 3, 0), (0, 4, 0), (3, 5, 2), (4, 6, 1)][:n]
    assert ent.dtype == _hip.BASES_DTYPE and ent.tolist() == want
    assert pool == (b"\x12\x34\x56" if nchunks == 2 else b"\x12\x34\x56\xab\xcd")
    assert CHUNKS[2][1][3][0]["off"].tolist() == [0, 1]  # (the chunks' own entries are left as they were)


def test_the_join_of_what_was_asked_for_and_of_nothing():
    col = mp.TokenisedChunks(edited=True)
    assert col.want == dict(edited=True)
    out = col.joined()
    assert sorted(out) == ["edits", "recs"] and out["edits"].dtype == _hip.EDIT_DTYPE and len(out["edits"]) == len(out["recs"]) == 0
    out = mp.TokenisedChunks(named=True, based=True).joined()
    assert out["names"][0] == b"" and out["names"][1].tolist() == [0]
    assert out["bases"][0].dtype == _hip.BASES_DTYPE and len(out["bases"][0]) == 0 and out["bases"][1] == b""
    assert sorted(mp.TokenisedChunks().joined()) == ["recs"]


def test_a_chunk_from_the_host_tokeniser_fills_the_same_lists():
    """Whatever was asked for comes from the host definitions through one call, in the order the device returns them."""
    line = "r1\t0\ta\t5\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:1\n"
    col = mp.TokenisedChunks(named=True, placed=True, edited=True, based=True)
    recs = mp.tokenise_sam([line], {"a": 0})
    col.add_from_host(recs, [line], ["r1"])
    out = col.joined()
    assert out["names"] == (b"r1", out["names"][1]) and out["names"][1].tolist() == [0, 2]
    assert out["places"].tolist() == [(4, 4)] and out["edits"].tolist() == [(1, 4)]
    assert out["bases"][0].tolist() == [(0, 4, 4)] and len(out["bases"][1]) == 2
    only = mp.TokenisedChunks(placed=True)
    only.add_from_host(recs, [line], ["r1"])
    assert sorted(only.joined()) == ["places", "recs"] and only.joined()["places"].tolist() == [(4, 4)]
