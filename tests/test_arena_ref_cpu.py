"""The host model of the level arena (arena_ref.py) on hand-worked sequences, and the seeded instances of test_gpu_capacity.py
against the oracle: each property a GPU test relies on is asserted here, so an edit that loses one fails this file on any machine."""
import pytest

import arena_ref
import capacity_cases as cc
from arena_ref import LevelArena


def test_a_run_that_exactly_fills_a_chunk_stays_in_it():
    a = LevelArena(8, 4)
    assert a.reserve(0, 5) == 0
    assert a.reserve(0, 3) == 5  # 5 + 3 == 8: fits
    assert a.peak == 1
    assert a.reserve(0, 1) == 8  # the chunk is full: the next run opens chunk 1
    assert a.peak == 2


def test_a_run_one_entry_too_long_for_the_remainder_opens_a_chunk():
    a = LevelArena(8, 4)
    assert a.reserve(0, 5) == 0
    assert a.reserve(0, 4) == 8  # 5 + 4 == 9: the remainder of 3 is abandoned
    assert a.reserve(0, 4) == 12
    assert a.reserve(0, 1) == 16  # 8 entries taken in chunk 1
    assert a.peak == 3


def test_a_run_of_a_whole_chunk():
    a = LevelArena(8, 3)
    assert a.reserve(2, 8) == 0
    assert a.reserve(2, 8) == 8
    assert a.reserve(2, 1) == 16
    assert a.reserve(2, 8) is None
    with pytest.raises(ValueError):
        a.reserve(2, 9)
    with pytest.raises(ValueError):
        a.reserve(2, 0)


def test_levels_interleave_one_open_chunk_each():
    a = LevelArena(8, 8)
    assert a.reserve(0, 3) == 0    # level 0 -> chunk 0
    assert a.reserve(1, 4) == 8    # level 1 -> chunk 1
    assert a.reserve(0, 3) == 3
    assert a.reserve(2, 8) == 16   # level 2 -> chunk 2
    assert a.reserve(1, 4) == 12
    assert a.reserve(1, 1) == 24   # level 1 full -> chunk 3
    assert a.reserve(0, 2) == 6    # level 0 still has exactly 2 left
    assert a.reserve(2, 1) == 32   # chunk 4
    assert a.peak == 5
    assert a.chunks == {0: [0], 1: [3, 1], 2: [4, 2]}


def test_reclaim_reuses_chunks_last_in_first_out():
    a = LevelArena(8, 8)
    for _ in range(3):
        a.reserve(0, 8)            # level 0 owns chunks 0, 1, 2 (head 2)
    assert a.reserve(1, 8) == 24   # chunk 3
    a.free_level(0)
    assert a.stack == [2, 1, 0]    # head first: the oldest chunk is on top
    assert a.reserve(1, 1) == 0    # chunk 0 again
    assert a.reserve(2, 1) == 8    # chunk 1
    a.free_level(1)                # level 1's list is 0 (head), 3
    assert a.stack == [2, 0, 3]
    assert a.reserve(3, 1) == 24 and a.reserve(4, 1) == 0 and a.reserve(5, 1) == 16
    assert a.reserve(6, 1) == 32   # the stack is empty: the next never-used chunk
    assert a.peak == 5
    a.free_level(7)                # a level without chunks
    assert a.stack == []


def test_exhaustion_returns_none_and_changes_nothing():
    a = LevelArena(8, 2)
    assert a.reserve(0, 6) == 0 and a.reserve(1, 6) == 8
    before = (dict(a.open), dict(a.used), {k: list(v) for k, v in a.chunks.items()}, list(a.stack), a.fresh, a.peak)
    assert a.reserve(0, 3) is None and a.reserve(2, 1) is None
    assert before == (a.open, a.used, a.chunks, a.stack, a.fresh, a.peak)
    assert a.reserve(0, 2) == 6    # what still fits is still served
    a.free_level(1)
    assert a.reserve(2, 1) == 8    # and a recycled chunk ends the shortage


def test_the_peak_survives_a_reset():
    a = LevelArena(4, 8)
    for d in range(3):
        a.reserve(d, 1)
    a.reset()
    assert a.peak == 3 and a.reserve(5, 4) == 0
    assert a.peak == 3


def test_prior_layout_by_hand():
    nodes = [(0, 3), (1, 4), (1, 0), (1, 5), (2, 8), (1, 1), (0, 1)]  # chunk 8
    offs, chunks = arena_ref.prior_layout(nodes, 8)
    assert offs == [0, 8, None, 16, 24, 21, 3] and chunks == 4
    # a move after three nodes kills level 0: its chunk serves the next level that needs one
    offs, chunks = arena_ref.prior_layout(nodes[:6], 8, moves=[3])
    assert offs == [0, 8, None, 0, 16, 5] and chunks == 3
    # one chunk short: the first run that finds no chunk, and every later one, has no offset
    offs, chunks = arena_ref.prior_layout(nodes, 8, n_chunks=3)
    assert offs == [0, 8, None, 16, None, None, None] and chunks == 3


def test_visited_growth_series_and_bounds():
    assert arena_ref.visited_consumed(10, 0) == (0, 0)
    assert arena_ref.visited_consumed(10, 1) == (2, 2) and arena_ref.visited_consumed(10, 2) == (2, 2)
    assert arena_ref.visited_consumed(10, 3) == (6, 4) and arena_ref.visited_consumed(10, 5) == (14, 8)
    assert arena_ref.visited_consumed(10, 9) == (24, 10)  # 2 + 4 + 8 + 10: the cap is n_valid
    assert arena_ref.visited_consumed(1, 1) == (1, 1) and arena_ref.visited_consumed(3, 3) == (5, 3)
    # level 0: 24 entries, largest block 10; level 1: 2 + 6 = 8 entries, largest block 4; chunk 16
    nodes = [(0, 10, 9), (1, 10, 1), (1, 10, 3), (2, 0, 0), (2, 5, 0)]
    assert arena_ref.visited_bounds(nodes, 16) == (2 + 1, 4 + 1)  # ceil(24 / 16), ceil(24 / 7); ceil(8 / 16), ceil(8 / 13)


# ---- the seeded instances of the GPU tests ------------------------------------------------------------------------------------------
def test_single_slot_instances_open_several_chunks():
    for inst, sims in ((cc.SINGLE, cc.SMALL[3]), (cc.WIDE, cc.WIDE_SIMS)):
        d = cc.auto_episode(inst, sims)
        assert d["n_nodes"] > 50 and len(d["actions"]) >= 6
        assert d["P"] >= 3, "the engine never builds fewer than 2 chunks: one short of P must still be a legal size"
        lo, hi = d["visited"]
        assert 3 <= lo <= hi
        assert all(o is not None for o, nd in zip(d["offsets"], d["nodes"]) if nd[1] > 0)
        assert sum(1 for nd in d["nodes"] if nd[1] == 0) > 0, "terminal nodes (which reserve nothing) are part of the case"
        assert len({o for o in d["offsets"] if o is not None}) == sum(1 for o in d["offsets"] if o is not None)


def test_exact_fill_instance_ends_a_run_on_a_chunk_boundary():
    d = cc.exact_fill_search()
    chunk = max(cc.PCHUNK_MIN, cc.EXACT_FILL[0] * cc.EXACT_FILL[2])
    level1 = [(off, nd[1]) for off, nd in zip(d["offsets"], d["nodes"]) if nd[0] == 1]
    assert len(level1) == cc.EXACT_FILL[3] - 1 and all(n == 128 for _, n in level1)
    first = level1[0][0]
    assert first % chunk == 0 and [off for off, _ in level1[:32]] == [first + 128 * k for k in range(32)]  # the 32nd run ends the chunk
    assert level1[32][0] % chunk == 0 and level1[32][0] != first  # and the 33rd opens the next one
    assert d["P"] == 3


def test_reclaim_instance_needs_fewer_chunks_with_reclaim():
    d = cc.external_episode(cc.RECLAIM, cc.SMALL[3])
    assert 3 <= d["P_reclaim"] < d["P"]
    assert len(d["moves_at"]) == len(d["actions"]) and d["moves_at"][-1] == d["n_nodes"]
    assert d["actions"] == cc.auto_episode(cc.RECLAIM, cc.SMALL[3])["actions"]  # driven move by move it is the same episode


def test_isolation_instances_have_one_strictly_neediest():
    eps = [cc.auto_episode(inst, cc.SMALL[3]) for inst in cc.ISOLATION]
    assert len(eps) == 5 and cc.NEEDIEST == 2, "the slot that overflows is never the last one"
    others = [e for k, e in enumerate(eps) if k != cc.NEEDIEST]
    need = eps[cc.NEEDIEST]
    for what in ("n_nodes", "P"):
        cap = max(e[what] for e in others)
        assert need[what] > cap >= 3, what
    cap = max(e["visited"][1] for e in others)  # enough for every other slot whatever the packing ...
    assert need["visited"][0] > cap >= 3        # ... and too little for the neediest whatever the packing
    fit = [eps[k] for k in cc.RECOVERY]
    assert len(fit) == 5 and cc.NEEDIEST not in cc.RECOVERY


def test_ring_pool_finishes_more_episodes_than_the_ring_holds():
    eps = cc.tiny_episodes()
    assert len({e["wh"].tobytes() for e in eps}) == cc.TINY_DISTINCT == 8
    assert all(1 <= len(e["actions"]) <= cc.TINY[2] for e in eps)  # every instance is an episode with a record
    assert len({(tuple(e["actions"]), e["outcome"], e["score"]) for e in eps}) > 4, "records that tell the instances apart"
    # every instance of the pool ends in a record (an episode cannot fail at these sizes), so the pool's size is what overflows the ring
    assert cc.RING_POOL == cc.RING_CAP + 6 and cc.RING_CAP == max(4 * cc.RING_SLOTS, 1024) and cc.RING_POOL > cc.TINY_DISTINCT


def test_replay_pool_tells_a_stale_index():
    eps = [cc.auto_episode(inst, cc.REPLAY_SIMS) for inst in cc.REPLAY_POOL]
    last, prev = eps[-1], eps[-2]
    assert last["outcome"] != prev["outcome"] and last["outcome"] != 0 and prev["outcome"] != 0
    assert len(prev["actions"]) >= len(last["actions"]) >= 2
    assert sum(len(e["actions"]) for e in eps[:-1]) >= 2
