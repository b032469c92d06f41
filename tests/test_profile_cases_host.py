"""tests/profile_cases.py proved on the host: the sequential Python definition equals the C oracle on every case it is used for
(whole and cut into shards), the model agrees with both, every family reaches the edge of k_profile_pass / k_bins_reduce it is
named after, and the constants the cases are aimed with are the ones in metalign_amd/csrc/mg_profile.hip."""
import os
import re

import numpy as np
import pytest

import profile_cases as pc
from profile_cases import HALO, ITEMS, M_DROP, M_IDENT, M_KEEP, M_SWAP, PB, QLIM, STAGED, TILE, WIN_TILES

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metalign_amd", "csrc", "mg_profile.hip")
KEYS = ("count", "bases", "first_seen", "tot_rds", "n_ambig", "mm_offsets", "mm_tax", "mm_hitlen", "mm_read")
SMALL = [(f, n) for f, n in pc.ALL if f in ("halo_edges", "thread_and_wave_edges", "mode_edges")
         or n in ("undecided", "tile_maps", "shard_args", "hashed_knob_full", "hashed_natural_full", "first_seen_direct", "first_seen_hashed")
         or n.startswith("bypass") or n in ("blocked64", "blocked63", "crowded8", "chain2_kept", "chain2_dropped", "hashed_knob_16",
                                            "hashed_natural_16")]


def _read_of(m, pos):
    i = int(np.searchsorted(m.starts, pos))
    assert m.starts[i] == pos, "no read starts at the mark"
    return i


def _sharded_definition(c, cuts):
    """The stream cut at `cuts`, shard by shard through the Python definition -> the whole stream's result, and the shards'."""
    parts = [(p, n, look and n > 0) for p, n, look in pc.shards(c, cuts)]   # (an empty shard is nothing, its lookahead included)
    maps = [tuple(pc.define_shard(c, p, n, look, x, False, 0)["state_end"] for x in (0, 1)) if n else (0, 1) for p, n, look in parts]
    res, x, base, first = [], 1, 0, True
    for (p, n, look), mp in zip(parts, maps):
        r = pc.define_shard(c, p, n, look, x, first and n > 0, base)
        r["incoming"], r["map"] = x, mp
        res.append(r)
        first = first and n == 0
        base += r["groups"]
        x = mp[x]
    return res


def _merge(c, res):
    mm = [pc.mm_of(r) for r in res]
    off = [np.zeros(1, np.uint64)]
    tot = 0
    for o, t, _, _ in mm:
        off.append(o[1:] + np.uint64(tot))
        tot += len(t)
    first = np.minimum.reduce([r["first_seen"] for r in res])
    return dict(count=sum(r["count"] for r in res), bases=sum(r["bases"] for r in res), first_seen=first,
                tot_rds=sum(r["groups"] for r in res), n_ambig=sum(r["ambig"] for r in res), mm_offsets=np.concatenate(off),
                mm_tax=np.concatenate([m[1] for m in mm]), mm_hitlen=np.concatenate([m[2] for m in mm]),
                mm_read=np.concatenate([m[3] for m in mm]))


def _equal(got, want, what):
    for key in KEYS:
        assert np.array_equal(np.asarray(got[key]).astype(np.uint64), np.asarray(want[key]).astype(np.uint64)), (what, key)


def test_case_names_are_the_builders():
    for fam in pc.FAMILIES:
        assert list(pc.family(fam)) == pc.NAMES[fam], fam
        assert all(c.family == fam for c in pc.family(fam).values())
    assert set(SMALL) == {(f, n) for f, n in pc.ALL if len(pc.case(f, n).recs) <= pc.PY_LIMIT}


@pytest.mark.parametrize("fam,name", SMALL)
def test_python_definition_equals_the_oracle(oracle_lib, fam, name):
    """... whole and cut into shards (the whole-stream version of every sharded case), and the model agrees read by read."""
    c = pc.case(fam, name)
    want = oracle_lib.profile_assign(c.recs, c.ref2tax, c.ntax, pc.PCT_ID)
    for cuts in c.cuts:
        res = _sharded_definition(c, cuts)
        _equal(_merge(c, res), want, cuts)
        for (part, n, look), r in zip(pc.shards(c, cuts), res):
            if n == 0:
                continue
            m = pc.model(part, c.ref2tax, n, look, incoming=r["incoming"])
            assert [3 if k < 0 else int(k) for k in m.kind] == [v[0] for v in r["verdicts"]], (name, cuts)
            assert m.shard_map == r["map"] and len(m.starts) == r["groups"]
            assert m.tile_reads.sum() == r["groups"] and m.tile_mm.sum() == len(r["mm"])
            assert m.tile_entries.sum() == sum(len(t) for _, t, _ in r["mm"])
    for inc, first, base in c.shard_args or ():
        r = pc.define_shard(c, c.recs, len(c.recs), False, inc, first, base)
        m = pc.model(c.recs, c.ref2tax, incoming=inc)
        assert [3 if k < 0 else int(k) for k in m.kind] == [v[0] for v in r["verdicts"]]
        if (inc, first, base) == (1, 1, 0):
            _equal(_merge(c, [r]), want, "shard_args")


@pytest.mark.parametrize("fam,name", [fn for fn in pc.ALL if fn not in SMALL and (not fn[1].startswith("mixed") or fn[1].endswith("grid0"))])
def test_model_equals_the_oracle_on_the_large_streams(oracle_lib, fam, name):
    """Above PY_LIMIT records the model is what the shards' maps are compared with: its totals are the oracle's."""
    c = pc.case(fam, name)
    want = oracle_lib.profile_assign(c.recs, c.ref2tax, c.ntax, pc.PCT_ID)
    m = pc.model(c.recs, c.ref2tax)
    assert len(m.starts) == want["tot_rds"] and int((m.kind == 0).sum()) + 1 == want["n_ambig"]
    assert m.tile_mm.sum() == len(want["mm_hitlen"]) and m.tile_entries.sum() == len(want["mm_tax"])
    assert np.array_equal(np.nonzero(m.kind == 2)[0], want["mm_read"].astype(np.int64))
    assert int((m.kind == 1).sum()) == int(want["count"].sum())
    assert m.tile_reads.max() < 1 << pc.TILE_COUNTER_BITS and m.tile_mm.max() < 1 << pc.TILE_COUNTER_BITS


# ---------------------------------------------------------------- what each family reaches
def test_halo_edges_reach_both_sides_of_the_staged_window():
    seen = set()
    for lead in pc.HALO_LEADS:
        for kind in pc.HALO_KINDS:
            for dropped in (0, 1):
                c = pc.case("halo_edges", "lead%d_%s_%s" % (lead, kind, "dropped" if dropped else "kept"))
                assert len(c.recs) <= pc.PY_LIMIT
                m = pc.model(c.recs, c.ref2tax)
                for mark, pos in c.marks.items():
                    i = _read_of(m, pos)
                    assert m.lead[i] == lead and m.state_in[i] == dropped and m.read_map[i - 1] == (M_DROP if dropped else M_KEEP)
                    idx = m.close[i] - m.tile[i] * TILE   # staged index of the closing line
                    if mark.startswith("close"):
                        assert idx == int(mark[5:]) and bool(m.staged[i]) == (idx < STAGED)
                    else:
                        assert m.close[i] - pos == int(mark[3:]) and not m.staged[i] and idx >= STAGED + TILE // 4
                    assert bool(m.classify3[0][i]) == (kind == "pair") == bool(m.classify3[1][i])
                    assert m.kind[i] == {"uniq": 1, "mm": 2, "pair": 1 if dropped else 2}[kind]
                    if kind != "uniq":   # the dropped first line is a list entry less (mm) or another verdict (pair)
                        assert (m.kinds[0][i], m.nmm[0][i]) != (m.kinds[1][i], m.nmm[1][i])
                    seen.add((lead, int(idx) if idx < 3000 else "far", kind, dropped))
                assert len(c.marks) == len(pc.HALO_CLOSES) + len(pc.HALO_FAR)
    assert len(seen) == len(pc.HALO_LEADS) * 5 * 3 * 2
    assert set(pc.HALO_CLOSES) == {STAGED - 2, STAGED - 1, STAGED, STAGED + 1} and STAGED == TILE + HALO
    assert set(pc.HALO_LEADS) >= {0, ITEMS - 1, ITEMS, TILE - ITEMS, TILE - 1}


def test_halo_tails_end_at_the_tile_multiple():
    for d in (-1, 0, 1):
        for tag in ("short", "long"):
            for kind in ("mm", "pair"):
                c = pc.case("halo_edges", "tail%+d_%s_%s" % (d, tag, kind))
                (nrecs,), (_, again) = c.cuts
                assert nrecs == 2 * TILE + d and again == nrecs   # (the second cut list holds an empty shard)
                part, n, look = pc.shards(c, (nrecs,))[0]
                m = pc.model(part, c.ref2tax, n, look)
                i = _read_of(m, c.marks["last"])
                assert i == len(m.starts) - 1 and m.close[i] == nrecs and bool(m.staged[i]) == (tag == "short")
                assert m.ntiles == (3 if d == 1 else 2) and m.kind[i] == 2 and bool(m.classify3[0][i]) == (kind == "pair")
                nl = pc.case("halo_edges", "tail%+d_%s_%s_nolook" % (d, tag, kind))
                assert len(nl.recs) == nrecs
                m = pc.model(nl.recs, nl.ref2tax)
                assert m.close[-1] == -1 and m.kind[-1] == -1
                assert pc.define_shard(nl, nl.recs, nrecs, False, 1, True, 0)["verdicts"][-1] == (3, 0, 0)


def test_thread_and_wave_edges():
    c = pc.case("thread_and_wave_edges", "edges")
    m = pc.model(c.recs, c.ref2tax)
    for t in pc.EDGE_THREADS:
        i = _read_of(m, c.marks["next%d" % t])
        assert m.lead[i] == ITEMS * t + ITEMS - 1 and m.close[i] == m.starts[i] + 1 and m.close[i] % ITEMS == 0
        assert (m.close[i] // TILE != m.tile[i]) == (t == PB - 1)
        i = _read_of(m, c.marks["skip%d" % t])
        assert m.lead[i] == ITEMS * t + ITEMS - 1 and m.close[i] == m.starts[i] + ITEMS + 1
        assert (m.close[i] % TILE) // ITEMS == (t + 2) % PB and m.close[i] % ITEMS == 0 and m.kind[i] == 2
    assert {t // 64 for t in pc.EDGE_THREADS} == {0, 1, 2, 3} and {63, 127, 191, 255} <= set(pc.EDGE_THREADS)
    t = c.marks["singles"] // TILE
    assert c.marks["singles"] % TILE == 0 and m.tile_reads[t] == TILE
    t = c.marks["inside"] // TILE + 1
    assert m.tile_reads[t] == 0 and m.tile_map[t] == M_IDENT and m.tile_reads[t - 1] > 0 and m.tile_reads[t + 1] > 0
    t = c.marks["pairs"] // TILE
    assert m.tile_reads[t] == TILE // 2 == m.tile_mm[t] and m.tile_entries[t] == TILE and m.tile_mm[t] < 1 << pc.TILE_COUNTER_BITS
    assert set(np.unique(m.thread_map)) >= {M_IDENT, M_KEEP, M_DROP}


def test_state_chains_are_decided_far_behind():
    for nt in pc.CHAIN_TILES:
        for dropped in (0, 1):
            c = pc.case("state_chains", "chain%d_%s" % (nt, "dropped" if dropped else "kept"))
            m = pc.model(c.recs, c.ref2tax)
            assert m.ntiles == nt and np.all(m.tile_map[1:] == M_IDENT) and np.all(m.read_map[1:] == M_IDENT)
            assert np.all(m.decided_by[1:] == 0) and np.all(m.tile_state_in[1:] == dropped)   # tile nt - 1 is decided by tile 0
            assert np.all(m.kind[:-1] == 0) if dropped else np.all(m.kind[:-1] > 0)
            assert (m.tile_mm[1:] > 0).all() != bool(dropped)   # the counts depend on the far decision, not only the verdicts
    # both sides of every look-back round: the window is WIN_TILES tiles, tile t's first window ends at tile t - WIN_TILES
    assert {WIN_TILES - 1, WIN_TILES, WIN_TILES + 1, WIN_TILES + 2, 2 * WIN_TILES - 1, 2 * WIN_TILES, 2 * WIN_TILES + 1} <= set(pc.CHAIN_TILES)
    assert max(pc.CHAIN_TILES) == 600
    c = pc.case("state_chains", "undecided")
    m0, m1 = pc.model(c.recs, c.ref2tax, incoming=0), pc.model(c.recs, c.ref2tax, incoming=1)
    assert np.all(m0.read_map == M_IDENT) and np.all(m1.kind[:-1] == 0) and np.all(m0.kind[:-1] > 0) and m0.tile_mm.min() > 0


def test_tile_maps_and_probes():
    c = pc.case("state_chains", "tile_maps")
    m = pc.model(c.recs, c.ref2tax)
    want = [c.marks["map_tile%d" % t] for t in range(1, m.ntiles - 1)]
    assert list(m.tile_map[1:m.ntiles - 1]) == want and set(want) == {M_IDENT, M_KEEP, M_DROP, M_SWAP}
    assert len({(a, b) for a, b in zip(want, want[1:])}) >= 12   # most ordered pairs of maps meet at a tile boundary
    for t in range(1, m.ntiles - 1):   # no thread of the tile carries the tile's map alone
        th = m.thread_map[t * PB:(t + 1) * PB]
        assert (th != M_IDENT).sum() >= 2
    for probe, d in pc.PROBES:
        for dropped in (0, 1):
            c = pc.case("state_chains", "probe%d_d%d_%s" % (probe, d, "dropped" if dropped else "kept"))
            m = pc.model(c.recs, c.ref2tax)
            dec = c.marks["decider"] // TILE
            assert dec == probe - d and m.decided_by[probe] == dec and m.tile_state_in[probe] == dropped
            assert m.tile_map[dec] == (M_DROP if dropped else M_KEEP) and m.tile_state_in[dec] == 1 - dropped
            assert np.all(m.tile_map[dec + 1:] == M_IDENT) and np.all(m.tile_map[2:dec] == M_IDENT)
            assert m.tile_mm[probe] > 0 if not dropped else m.tile_mm[probe] == 0
    assert {d for _, d in pc.PROBES} >= {1, WIN_TILES - 1, WIN_TILES, WIN_TILES + 1} and max(d for _, d in pc.PROBES) > 2 * WIN_TILES
    c = pc.case("state_chains", "shard_args")
    m = pc.model(c.recs, c.ref2tax)
    assert set(np.unique(m.read_map)) == {0, 1, 2, 3} and m.classify3[0].any() and m.tile_mm.sum() > 0
    assert {g for _, _, g in c.shard_args} == {0, 1, 2**32 - 1, 2**32, 2**40} and len(c.shard_args) == 20


def test_grids_and_ticket_lanes():
    for nt in (40, 300):
        c = pc.case("grid_and_tickets", "mixed%d_grid0" % nt)
        m = pc.model(c.recs, c.ref2tax)
        assert m.ntiles == nt and set(np.unique(m.read_map)) == {0, 1, 2, 3} and len(set(np.unique(m.tile_map))) >= 3
        assert m.classify3[0].any() and (m.tile_mm > 0).sum() >= nt // 2 and (m.tile_map != M_IDENT).sum() >= nt // 2
        assert len(c.cuts[1]) >= 2
        for g in pc.GRIDS:
            assert pc.case("grid_and_tickets", "mixed%d_grid%d" % (nt, g)).knobs == ({"k3_grid": g} if g else {})
            assert g < nt
    lanes = [min(pc.TICKET_LANES, g) for g in pc.GRIDS if g]
    assert set(lanes) == {1, 2, 15, 16} and any(g > pc.TICKET_LANES and g % pc.TICKET_LANES for g in pc.GRIDS)


def test_bin_fields_are_as_full_as_the_intervals_allow(oracle_lib):
    hist = lambda c: pc.hist_mode(c.ntax, bool(c.knobs.get("k3_hashed")))[0]  # noqa: E731
    c = pc.case("bin_fields", "direct_257")
    m = pc.model(c.recs, c.ref2tax)
    assert hist(c) == 1 and c.knobs["k3_grid"] == 1 and m.ntiles == pc.FLUSH_TILES + 1
    assert int((m.kind[m.tile < pc.FLUSH_TILES] == 1).sum()) == pc.FLUSH_TILES * TILE - 1 and len(np.unique(c.recs["ref_new"][:-1] & 0x7FFFFFFF)) == 1
    assert np.all(c.recs["flag_len"][1:-1] >> 12 == QLIM - 1) and pc.FLUSH_TILES * TILE * (QLIM - 1) < 1 << 40
    for name in ("hashed_knob_%d", "hashed_natural_%d"):
        for nt in (pc.HASH_FLUSH_TILES + 1, 2 * pc.HASH_FLUSH_TILES + 1):
            c = pc.case("bin_fields", name % nt)
            m = pc.model(c.recs, c.ref2tax)
            assert hist(c) == 2 and c.knobs["k3_grid"] == 1 and m.ntiles == nt and (c.ntax > pc.DIRECT_MAX_TAX) == ("natural" in name)
            if nt > 2 * pc.HASH_FLUSH_TILES:   # the second interval is full: 30720 reads of 16383 bases in one bin before the flush
                sel = (m.tile >= pc.HASH_FLUSH_TILES) & (m.tile < 2 * pc.HASH_FLUSH_TILES)
                assert int((m.kind[sel] == 1).sum()) == pc.HASH_FLUSH_TILES * TILE == 30720
    for name in ("hashed_knob_full", "hashed_natural_full"):   # ... and the first one, when the shard is entered kept
        c = pc.case("bin_fields", name)
        m = pc.model(c.recs, c.ref2tax, incoming=0)
        n = int((m.kind[m.tile < pc.HASH_FLUSH_TILES] == 1).sum())
        assert hist(c) == 2 and n == 30720 and all(a[0] == 0 for a in c.shard_args)
        assert n < 1 << pc.HASH_COUNT_BITS <= n + TILE and n * (QLIM - 1) < 1 << pc.HASH_BASES_BITS   # (one tile more overflows the count)
    for name in ("bypass_direct", "bypass_hashed", "bypass_natural"):
        c = pc.case("bin_fields", name)
        ln = c.recs["flag_len"][2:-1] >> 12
        assert set(ln[::2]) | set(ln[1::2]) == {QLIM - 1, QLIM} and set(ln[::2]) != set(ln[1::2])
        assert (int(c.recs["ref_new"][5]) & 0x7FFFFFFF) % 2 == 0   # (a queued 2^14 would spill into the taxon's lowest bit)
    assert [hist(pc.case("bin_fields", n)) for n in ("bypass_direct", "bypass_hashed", "bypass_natural")] == [1, 2, 2]
    for name in ("first_seen_direct", "first_seen_hashed"):
        c = pc.case("bin_fields", name)
        want = oracle_lib.profile_assign(c.recs, c.ref2tax, c.ntax, pc.PCT_ID)
        m = pc.model(c.recs, c.ref2tax)
        i = _read_of(m, c.marks["after_dropped"])
        assert want["first_seen"][c.marks["t_first"]] == 0 and want["count"][c.marks["t_first"]] == 1
        assert m.state_in[i] == 1 and want["first_seen"][c.marks["t_dropped"]] == i and want["count"][c.marks["t_dropped"]] == 1
        assert want["first_seen"][c.marks["t_last"]] == want["tot_rds"] - 2 == _read_of(m, c.marks["last"])


def test_mode_edges(oracle_lib):
    modes = {n: pc.hist_mode(n) for n in pc.MODE_NTAX}
    assert modes == {1: (1, 3), 2048: (1, 3), 2049: (1, 3), 3413: (1, 3), 3414: (1, 2), 4096: (1, 2), 4097: (2, 3),
                     pc.HASH_MAX_TAX: (2, 3), pc.HASH_MAX_TAX + 1: (0, 3)}
    assert 3413 * 12 <= pc.LDS_TWO_PER_CU < 3414 * 12
    for n in pc.MODE_NTAX:
        c = pc.case("mode_edges", "ntax%d" % n)
        want = oracle_lib.profile_assign(c.recs, c.ref2tax, n, pc.PCT_ID)
        assert want["count"][0] > 0 and want["count"][n - 1] > 0 and len(want["mm_hitlen"]) > 0 and len(c.recs) < 5 * TILE
        assert want["bases"][0] >= QLIM   # (the queue bypass in every mode)


def test_the_model_composes_maps_in_order():
    """The model's vectorised composition against map_then applied read by read (the order matters: the maps do not commute)."""
    for fam, name in (("state_chains", "tile_maps"), ("state_chains", "shard_args"), ("thread_and_wave_edges", "edges")):
        c = pc.case(fam, name)
        m = pc.model(c.recs, c.ref2tax)
        tiles, threads, whole = [M_IDENT] * m.ntiles, [M_IDENT] * (m.ntiles * PB), M_IDENT
        for pos, mp in zip(m.starts.tolist(), m.read_map.tolist()):
            tiles[pos // TILE] = pc.compose(tiles[pos // TILE], mp)
            threads[pos // ITEMS] = pc.compose(threads[pos // ITEMS], mp)
            whole = pc.compose(whole, mp)
        assert tiles == m.tile_map.tolist() and threads == m.thread_map.tolist() and (whole & 1, whole >> 1) == m.shard_map
    assert pc.compose(M_SWAP, M_KEEP) != pc.compose(M_KEEP, M_SWAP)


def _tile0_taxa(c, m):
    sel = (m.tile == 0) & (m.kind == 1)
    st = m.starts[sel] + m.state_in[sel]   # the first kept line gives the taxon
    return list(dict.fromkeys((c.recs["ref_new"][st] & 0x7FFFFFFF).tolist()))


def test_hash_collisions_reach_the_probe_limits():
    p = pc.collision_plan()
    T, slots = p["T"], pc.probe_slots(p["T"])
    assert p["ntax"] > pc.DIRECT_MAX_TAX and pc.hist_mode(p["ntax"]) == (2, 3) and len(set(slots)) == pc.HASH_PROBE_FREE
    assert all(pc.probe_slots(b, 1)[0] == s and b != T for b, s in zip(p["blockers"], slots))
    for name, nblock, probes, lands in (("blocked64", 64, 64, None), ("blocked63", 63, 64, slots[63]), ("crowded8", 8, 8, None)):
        c = pc.case("hash_collisions", name)
        m = pc.model(c.recs, c.ref2tax)
        assert c.knobs == {"k3_grid": 1} and c.twice and hist_is_hashed(c)
        seen = _tile0_taxa(c, m)
        first_T = _read_of(m, c.marks["T"])
        assert T not in seen and m.tile[first_T] == 1 and m.kind[first_T] == 1 and c.recs["ref_new"][c.marks["T"]] & 0x7FFFFFFF == T
        for order in (seen, seen[::-1]):   # whatever order the tile's threads reach the table in
            table, over = pc.table_after(order, probes if name != "crowded8" else pc.HASH_PROBE_FREE)
            assert all(s in table for s in slots[:nblock])
            if name == "crowded8":
                assert len(seen) > pc.HASH_CROWDED   # more keys than the crowded limit ask for the table: 8 probes from here on
            else:
                assert not over and len(table) <= pc.HASH_CROWDED
            placed = next((s for s in slots[:probes] if s not in table), None)
            assert placed == lands   # T exhausts its probes (None: the private bins) or stays in LDS at its 64th slot
    q = pc.six_plan()
    c = pc.case("hash_collisions", "six_keys")
    assert len({pc.probe_slots(t, 1)[0] for t in q["six"]}) == 1 and len(set(q["six"])) == 6 > 4 and c.ntax == q["ntax"] and not c.knobs
    refs = (c.recs["ref_new"] & 0x7FFFFFFF).astype(np.int64)
    for j in range(1, pc.SIX_TILES):
        assert set(np.unique(refs[j * TILE:(j + 1) * TILE])) & set(q["six"]) == {q["six"][j % 6]}
    assert pc.SIX_TILES >= 6 * 32   # a thread of k_bins_reduce reads ceil(grid / 32) tables: six of them hold six keys


def hist_is_hashed(c):
    return pc.hist_mode(c.ntax, bool(c.knobs.get("k3_hashed")))[0] == 2


# ---------------------------------------------------------------- the constants, read back from the source text
def _source_constants():
    text = open(SRC).read()
    env = {}
    for name in ("kPB", "kItems", "kTile", "kHalo", "kStaged", "kTicketLanes", "kWin", "kWinTiles", "kQueueLenBits", "kQueueLenLimit",
                 "kHashSlots", "kHashProbe", "kFlushTiles", "kHashProbeFree", "kHashCrowded", "kHashFlushTiles", "kHashMaxTax"):
        mt = re.search(r"\b%s = ([^,;]+)[,;]" % name, text)
        assert mt, name
        expr = re.sub(r"(\d)(?:ull|u)\b", r"\1", mt.group(1)).replace("/", "//")
        env[name] = eval(expr, {"__builtins__": {}}, dict(env))  # noqa: S307 (arithmetic over the constants before it)
    return text, env


def test_constants_are_the_kernel_s():
    text, k = _source_constants()
    assert (k["kPB"], k["kItems"], k["kHalo"], k["kWin"], k["kTicketLanes"]) == (pc.PB, pc.ITEMS, pc.HALO, pc.WIN, pc.TICKET_LANES)
    assert (k["kTile"], k["kStaged"], k["kWinTiles"]) == (pc.TILE, pc.STAGED, pc.WIN_TILES)
    assert (k["kHashSlots"], k["kHashProbe"], k["kHashProbeFree"], k["kHashCrowded"]) == (pc.HASH_SLOTS, pc.HASH_PROBE, pc.HASH_PROBE_FREE, pc.HASH_CROWDED)
    assert (k["kFlushTiles"], k["kHashFlushTiles"], k["kHashMaxTax"], k["kQueueLenBits"]) == (pc.FLUSH_TILES, pc.HASH_FLUSH_TILES, pc.HASH_MAX_TAX, pc.QUEUE_LEN_BITS)
    assert k["kQueueLenLimit"] == pc.QLIM
    assert "base -= kLbWaves * 64 * kWin" in text and re.search(r"constexpr int kLbWaves = 1;", text)
    assert re.findall(r"tax \* (\d+)u;", text) == [str(pc.HASH_MULT)]
    assert "hh >> 21" in text and "((hh >> 10) & 2046u) | 1u" in text and "s_nkeys <= kHashCrowded ? kHashProbeFree : kHashProbe" in text
    assert re.search(r"p->ntax <= (\d+) \? 1u : p->ntax <= kHashMaxTax \? 2u : 0u", text).group(1) == str(pc.DIRECT_MAX_TAX)
    mt = re.search(r"lds > (\d+) \* (\d+) \? 2u : 3u", text)
    assert int(mt.group(1)) * int(mt.group(2)) == pc.LDS_TWO_PER_CU
    assert "sizeof(unsigned long long) + sizeof(uint32_t)" in text   # 12 bytes per bin
    hashed = re.search(r'static_assert\((.*?), "hashed bin fields"\)', text).group(1)
    assert [int(x) for x in re.findall(r"<< (\d+)\)", hashed)] == [pc.HASH_COUNT_BITS, pc.HASH_BASES_BITS]
    assert "kHashFlushTiles * kTile <" in hashed and "kHashFlushTiles * kTile * kQueueLenLimit <" in hashed
    tile = re.search(r'static_assert\((.*?), "tile counters are 13-bit fields in the published aggregate"\)', text).group(1)
    assert tile == "kTile < (1 << %d)" % pc.TILE_COUNTER_BITS
    assert "hitlen < kQueueLenLimit" in text and "++tiles_binned == A.flush_tiles" in text
    assert 'dbg("k3_grid")' in text and text.count('dbg("k3_grid")') == 2   # the map-only launch and the commit launch
