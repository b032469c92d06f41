"""-m gpu: stage C's chained scan (k_profile_pass, k_bins_reduce; mg_profile.hip) held to its definition at every tile, window,
halo, flush and hash edge (tests/profile_cases.py; what each family reaches is shown by test_profile_cases_host.py).

Every case goes through
  * hip.profile_assign (one shard, one commit pass), twice in a row where the case says so (the workgroups' private bins must be
    left as found);
  * profile_begin_dev -> state_map / ngroups (the map-only pass, compared with the definition BEFORE any commit) -> commit, whole
    and cut into shards at read starts around tile multiples (an empty shard among them): equal to the unsharded oracle;
  * the same through commit_assign, the verdict words compared with the sequential definition up to PY_LIMIT records.
Equality is exact for every output key; the multimapped CSR is compared row by row and entry by entry, i.e. in SAM order."""
import functools

import numpy as np
import pytest

import profile_cases as pc
from util import stage_c_sharded

pytestmark = pytest.mark.gpu
KEYS = ("count", "bases", "first_seen", "tot_rds", "n_ambig", "mm_offsets", "mm_tax", "mm_hitlen", "mm_read")
U64_MAX = 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def _want(fam, name):
    """The whole-stream definition of a case (the C oracle): computed once, shared by every test that needs it."""
    import oracle
    c = pc.case(fam, name)
    return oracle.profile_assign(c.recs, c.ref2tax, c.ntax, pc.PCT_ID)


@functools.lru_cache(maxsize=None)
def _shards_want(fam, name, cuts):
    """Per shard of the stream cut at `cuts`: (state map, reads, verdict words or None) — the sequential Python definition up to
    PY_LIMIT records, the model (held to the oracle by the host test) above."""
    c = pc.case(fam, name)
    small = len(c.recs) <= pc.PY_LIMIT
    out, x = [], 1
    for part, n, look in pc.shards(c, cuts):
        if n == 0:
            out.append(((0, 1), 0, np.zeros(0, np.uint64)))
            continue
        if small:
            rs = [pc.define_shard(c, part, n, look, inc, False, 0) for inc in (0, 1)]
            mp, groups, words = (rs[0]["state_end"], rs[1]["state_end"]), rs[0]["groups"], pc.verdict_words(rs[x])
        else:
            m = pc.model(part, c.ref2tax, n, look)
            mp, groups, words = m.shard_map, len(m.starts), None
        out.append((mp, groups, words))
        x = mp[x]
    return out


def _equal(got, want, what):
    for key in KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.uint64), np.asarray(want[key]).astype(np.uint64)), (what, key)


def _set(knobs, c):
    for key, value in c.knobs.items():
        knobs(key, value)


@pytest.mark.parametrize("fam,name", pc.ALL)
def test_whole_stream_equals_the_oracle(hip, oracle_lib, knobs, fam, name):
    c = pc.case(fam, name)
    _set(knobs, c)
    want = _want(fam, name)
    for run in range(2 if c.twice else 1):
        _equal(hip.profile_assign(c.recs, c.ref2tax, c.ntax, pc.PCT_ID), want, run)
    if name.endswith("_dropped") and name.startswith("chain"):   # one decision at record 0 and nothing but Ambiguous reads behind it
        assert want["n_ambig"] == want["tot_rds"] and not want["count"].any() and len(want["mm_read"]) == 0


@pytest.mark.parametrize("assign", [False, True], ids=["commit", "commit_assign"])
@pytest.mark.parametrize("fam,name", pc.ALL)
def test_shards_equal_the_oracle_and_their_maps_the_definition(hip, oracle_lib, knobs, fam, name, assign):
    c = pc.case(fam, name)
    _set(knobs, c)
    want = _want(fam, name)
    for cuts in c.cuts:
        info = {}
        got = stage_c_sharded(hip, c.recs, c.ref2tax, c.ntax, list(cuts), pc.PCT_ID, info=info, assign=assign)
        shards = _shards_want(fam, name, cuts)
        assert info["maps"] == [s[0] for s in shards] and info["groups"] == [s[1] for s in shards], cuts
        _equal(got, want, cuts)
        if assign:
            for i, (_, groups, words) in enumerate(shards):
                w = info["words"][i]
                assert len(w) == 2 * groups
                if words is not None:
                    assert np.array_equal(w, words), (cuts, i, np.nonzero(w != words)[0][:4])
            # (above PY_LIMIT records: every read's kind against the oracle's totals and its multimapped reads)
            kinds = np.concatenate([w[0::2] & np.uint64(3) for w in info["words"]] or [np.zeros(0, np.uint64)])
            assert int((kinds == 1).sum()) == int(want["count"].sum()) and int((kinds == 2).sum()) == len(want["mm_read"])
            assert int((kinds == 0).sum()) + 1 == want["n_ambig"] and int((kinds == 3).sum()) == 1
            assert np.array_equal(np.nonzero(kinds == 2)[0], want["mm_read"].astype(np.int64))


def _commit_one(hip, c, inc, first, base, assign):
    """The whole stream as ONE shard entered with `inc`, committed at group_base `base` -> (accumulators, CSR, map, reads, words)."""
    ntax = c.ntax
    d_r, d_t = hip.array(c.recs), hip.array(c.ref2tax)
    acc = hip.empty(3 * ntax + 2, np.uint64)
    host = np.zeros(3 * ntax + 2, dtype=np.uint64)
    host[2 * ntax:3 * ntax] = U64_MAX
    acc.upload(host)
    sh = hip.profile_begin_dev(d_r.ptr, len(c.recs), False, d_t.ptr, ntax, ntax, pc.PCT_ID)
    try:
        mp, groups = sh.state_map(), sh.ngroups
        args = (inc, first, base, acc.ptr, acc.ptr + 8 * ntax, acc.ptr + 16 * ntax, acc.ptr + 24 * ntax)
        words = None
        if assign:
            d_w = hip.empty(max(2 * groups, 2), np.uint64)
            sh.commit_assign(*args, d_w.ptr)
            words = d_w.download()[:2 * groups]
            d_w.free()
        else:
            sh.commit(*args)
        mm = sh.multimapped()
        return acc.download(), mm, mp, groups, words
    finally:
        sh.free()
        for d in (d_r, d_t, acc):
            d.free()


@pytest.mark.parametrize("assign", [False, True], ids=["commit", "commit_assign"])
@pytest.mark.parametrize("fam,name", [(f, n) for f, n in pc.ALL if n in ("shard_args", "hashed_knob_full", "hashed_natural_full")])
def test_incoming_first_shard_and_group_base(hip, knobs, fam, name, assign):
    """incoming x first_shard x group_base through profile_begin_dev / commit against the sequential definition of the shard."""
    c = pc.case(fam, name)
    _set(knobs, c)
    ntax = c.ntax
    maps = [pc.define_shard(c, c.recs, len(c.recs), False, x, False, 0)["state_end"] for x in (0, 1)]
    for inc, first, base in c.shard_args:
        r = pc.define_shard(c, c.recs, len(c.recs), False, inc, first, base)
        out, mm, mp, groups, words = _commit_one(hip, c, inc, first, base, assign)
        what = (inc, first, base)
        assert mp == tuple(maps) and groups == r["groups"], what
        assert np.array_equal(out[:ntax], r["count"]) and np.array_equal(out[ntax:2 * ntax], r["bases"]), what
        assert np.array_equal(out[2 * ntax:3 * ntax], r["first_seen"]), what
        assert (int(out[3 * ntax]), int(out[3 * ntax + 1])) == (r["groups"], r["ambig"]), what
        for got, want in zip(mm, pc.mm_of(r)):
            assert np.array_equal(got, want), what
        if assign:
            assert np.array_equal(words, pc.verdict_words(r)), what
