"""The tree arenas at their capacity limits and the device error paths, through the C ABI.  Everything is compared exactly: the
oracle's trees and episodes (oracle_lib), and the host model of the level arena (arena_ref.py) for where a node's legal-move run
lands, how many chunks an episode needs and which cap is the first that suffices.

A slot that is meant to overflow is never the context's last one: the slots' slabs lie back to back in one allocation, so a guard
that is off by one shows as a neighbour's tree differing from the oracle's, not as an access outside the allocation.  The
single-episode tests therefore run their episode in the middle slot of three, the other two stay idle.

Two device error codes cannot be reached through the ABI and are not tried.  ERR_TABLE_FULL: the transposition table has at least
2 * node_cap slots and a lookup that finds it full makes the node arena's check report first.  ERR_PATH is only ever the second
error behind a capacity error (the simulation that could not get its node or block is abandoned), and the first error recorded is
the one reported: the isolation tests pin that the code reported is the arena's.
"""
import ctypes as C

import numpy as np
import pytest

import arena_ref
import capacity_cases as cc
import oracle_lib as orc
from engine_util import assert_trees_equal, host_evaluator, run_until_idle, tree_as_dict

pytestmark = pytest.mark.gpu

NODE, PRIOR, VISITED, RING, REPLAY = "node arena", "legal-move arena", "visited-edge arena", "finished-episode ring", "replay buffer"
MID = 1  # the slot of the single-episode tests


def lib():
    from resource_packing_self_play_amd import _lib
    return _lib


def evaluator(inst):
    return host_evaluator(lambda s: cc.KIND, inst[0] * inst[2], lambda s: cc.SALT)


def make_engine(inst, games, sims, rule=None, **kw):
    L = lib()
    W, H, N = inst[:3]
    eng = L.Engine(W, H, N, games, sims, cpuct=1.0, alpha=0.75, move_rule=L.MOVE_ARGMAX_FIRST if rule is None else rule, tie_salt=cc.SALT, **kw)
    eng.set_rank_buffer(cc.BUF)
    return eng


def arena_peak(eng):
    """rp_arena_peak -> (legal-move chunks, visited chunks, entries per legal-move chunk, entries per visited chunk)."""
    a, b, ce = C.c_int32(0), C.c_int32(0), (C.c_int32 * 2)()
    eng._ck(eng.L.rp_arena_peak(eng.h, C.byref(a), C.byref(b), ce))
    return a.value, b.value, ce[0], ce[1]


_chunks = {}


def chunk_sizes(inst):
    """The chunk sizes of this geometry, as rp_arena_peak reports them."""
    if inst[:3] not in _chunks:
        eng = make_engine(inst, 1, 1)
        _chunks[inst[:3]] = arena_peak(eng)[2:]
        eng.close()
    return _chunks[inst[:3]]


def ample(inst):
    pchunk, vchunk = chunk_sizes(inst)
    return dict(node_cap=1000, edge_cap=16 * pchunk, vis_cap=16 * vchunk)


def run_collecting_errors(eng, evaluate, limit=16):
    """run_until_idle to the end; every EngineError on the way is kept and the run goes on."""
    errors = []
    for _ in range(limit):
        try:
            run_until_idle(eng, evaluate)
            return errors
        except lib().EngineError as e:
            errors.append(e)
    raise AssertionError("the engine kept reporting errors: %s" % errors)


def assert_capacity(err, what):
    assert err.code == lib().ERR_CAPACITY and what in str(err), str(err)


def engine_keys(d):
    return [(np.ascontiguousarray(d["node_rows"][i]).tobytes(), np.ascontiguousarray(d["node_rem"][i]).tobytes()) for i in range(len(d["node_term"]))]


def assert_slot_equals_oracle(eng, g, ep, where=""):
    """The slot's complete tree, and the engine's node i is the oracle's i-th node: both create a node at its state's first sight
    (oracle: lookup(create) on entry to search; engine: materialize when an edge is traversed first), so creation order is the id."""
    d = eng.dump_tree(g)
    assert_trees_equal(tree_as_dict(d), ep["dump"], where)
    assert engine_keys(d) == ep["keys"], where + ": node ids are not the oracle's creation order"
    return d


def assert_records(eng, want, trace=True):
    """pop_finished returns exactly the episodes of `want` ({episode id: oracle episode}), each with the oracle's outcome, score and
    moves and -- with the trace -- its actions, the rows every move filled and the final bin."""
    rec = eng.pop_finished(packings=True) if trace else eng.pop_finished()
    ids = [int(i) for i in rec[0]]
    assert sorted(ids) == sorted(want), (sorted(ids)[:8], sorted(want)[:8])
    for k, i in enumerate(ids):
        ep = want[i]
        n = len(ep["actions"])
        assert (int(rec[1][k]), float(rec[2][k]), int(rec[3][k])) == (ep["outcome"], ep["score"], n), i
        if trace:
            N = rec[4].shape[1]
            assert rec[4][k].tolist() == ep["actions"] + [0] * (N - n), i
            assert [int(x) for x in rec[5][k]] == ep["filled"] + [0] * (N - n), i
            assert np.array_equal(rec[6][k], ep["board"]), i
    return ids


def play_single(inst, sims, **caps):
    """One episode in the middle slot of three -> the engine, not yet checked."""
    eng = make_engine(inst, 3, sims, **caps)
    eng.set_trace(True)
    wh = cc.items_of(inst)
    eng.begin_episodes(wh[None], [inst[0] * inst[1]], first=MID, episode_id=[77])
    return eng


def assert_single_matches(eng, ep):
    assert eng.status()[0].tolist() == [lib().PHASE_IDLE, lib().PHASE_EPISODE_DONE, lib().PHASE_IDLE]
    assert_records(eng, {77: ep})
    d = assert_slot_equals_oracle(eng, MID, ep)
    eng.check()
    return d


def assert_single_overflows(eng, inst, what):
    """The run raises RP_ERR_CAPACITY naming the arena, once; the slot is left RP_PHASE_FAILED and nothing finished."""
    errors = run_collecting_errors(eng, evaluator(inst))
    assert len(errors) == 1
    assert_capacity(errors[0], what)
    eng.check()
    assert eng.status()[0].tolist() == [lib().PHASE_IDLE, lib().PHASE_FAILED, lib().PHASE_IDLE]
    assert len(eng.pop_finished()[0]) == 0


def test_node_cap_exact_and_one_short():
    inst, sims = cc.SINGLE, cc.SMALL[3]
    ep = cc.auto_episode(inst, sims)
    caps = ample(inst)
    eng = play_single(inst, sims, **dict(caps, node_cap=ep["n_nodes"]))
    run_until_idle(eng, evaluator(inst))
    assert_single_matches(eng, ep)
    assert eng.tree_size(MID)[0] == ep["n_nodes"]
    eng.close()
    eng = play_single(inst, sims, **dict(caps, node_cap=ep["n_nodes"] - 1))
    assert_single_overflows(eng, inst, NODE)
    eng.close()


@pytest.mark.parametrize("inst,sims", [(cc.SINGLE, cc.SMALL[3]), (cc.WIDE, cc.WIDE_SIMS)], ids=["10x10", "33x12-64bit-rows"])
def test_legal_move_arena_layout_peak_and_exact_cap(inst, sims):
    """Without reclaim: every node's run lies where the model puts it, the reported peak is the model's chunk count P, P chunks are
    enough and P - 1 are not."""
    ep = cc.auto_episode(inst, sims)
    caps = ample(inst)
    pchunk, _ = chunk_sizes(inst)
    offs, P = arena_ref.prior_layout(ep["nodes"], pchunk)
    assert P >= 3
    for edge_cap in (caps["edge_cap"], P * pchunk):
        eng = play_single(inst, sims, **dict(caps, edge_cap=edge_cap))
        run_until_idle(eng, evaluator(inst))
        d = assert_single_matches(eng, ep)
        for i, (nd, off) in enumerate(zip(ep["nodes"], offs)):
            assert int(d["node_n_valid"][i]) == nd[1], i
            if nd[1] > 0:
                assert int(d["node_edge_off"][i]) == off, "node %d (level %d, %d legal moves)" % (i, nd[0], nd[1])
        assert arena_peak(eng)[0] == P
        eng.close()
    eng = play_single(inst, sims, **dict(caps, edge_cap=(P - 1) * pchunk))
    assert_single_overflows(eng, inst, PRIOR)
    eng.close()


def test_a_run_that_exactly_fills_its_chunk_stays_in_it():
    """The guard `used + need > chunk` at equality: 39 runs of 128 legal moves at level 1, the 32nd ends on the chunk's last entry
    (capacity_cases.EXACT_FILL).  Every run lies where the model puts it, the peak is 3 chunks, 3 chunks are enough and 2 are not."""
    L = lib()
    W, H, N, sims = cc.EXACT_FILL
    inst = (W, H, N)
    ref = cc.exact_fill_search()
    pchunk, vchunk = chunk_sizes(inst)
    offs, P = arena_ref.prior_layout(ref["nodes"], pchunk)
    assert P == 3 and offs[32] + 128 == 2 * pchunk and offs[33] == 2 * pchunk  # node 0 is the root: chunk 0; level 1 fills chunk 1
    evaluate = host_evaluator(lambda s: "uniform", W * N, lambda s: cc.SALT)
    for n_chunks in (16, P, P - 1):
        eng = make_engine(inst, 3, sims, rule=L.MOVE_EXTERNAL, node_cap=100, edge_cap=n_chunks * pchunk, vis_cap=16 * vchunk)
        eng.begin_episodes(ref["wh"][None], [N], first=MID)
        if n_chunks < P:
            errors = run_collecting_errors(eng, evaluate)
            assert len(errors) == 1
            assert_capacity(errors[0], PRIOR)
            assert eng.status()[0].tolist() == [L.PHASE_IDLE, L.PHASE_FAILED, L.PHASE_IDLE]
            assert eng.tree_size(MID)[0] == 33  # the root and the 32 children that filled the chunk
        else:
            run_until_idle(eng, evaluate)
            assert np.array_equal(eng.root_counts(MID, 1)[0], ref["counts"])
            d = assert_slot_equals_oracle(eng, MID, ref)
            assert [int(x) for x in d["node_edge_off"]] == offs and [int(x) for x in d["node_n_valid"]] == [nd[1] for nd in ref["nodes"]]
            assert arena_peak(eng)[0] == P
        eng.check()
        eng.close()


def test_legal_move_arena_with_reclaim():
    """reclaim = 1, moves played from outside against the oracle's visit counts: the node count after every move gives the model the
    interleaving of node creation and moves.  The peak is the model's, it is below the peak without reclaim, P_reclaim chunks are
    enough and one fewer is not.  (A tree whose dead levels have been recycled cannot be dumped, so the layout itself is checked
    without reclaim only.)"""
    L = lib()
    inst, sims = cc.RECLAIM, cc.SMALL[3]
    W, H, N = inst[:3]
    ep = cc.external_episode(inst, sims)
    caps = ample(inst)
    pchunk, _ = chunk_sizes(inst)

    def play(edge_cap):
        eng = make_engine(inst, 3, sims, rule=L.MOVE_EXTERNAL, reclaim=1, **dict(caps, edge_cap=edge_cap))
        eng.begin_episodes(ep["wh"][None], [W * H], first=MID)
        sizes, ended = [], 0
        try:
            for mv, a in enumerate(ep["actions"]):
                run_until_idle(eng, evaluator(inst))
                assert np.array_equal(eng.root_counts(MID, 1)[0], ep["counts"][mv]), mv
                ended = int(eng.advance_roots([a], first=MID)[0][0])
                sizes.append(eng.tree_size(MID)[0])
        except L.EngineError:
            assert eng.status()[0].tolist() == [L.PHASE_IDLE, L.PHASE_FAILED, L.PHASE_IDLE]
            eng.check()  # reported once
            eng.close()
            raise
        assert ended != 0
        return eng, sizes

    eng, sizes = play(caps["edge_cap"])
    assert sizes == ep["moves_at"]
    P = arena_ref.prior_layout(ep["nodes"], pchunk)[1]
    P_reclaim = arena_ref.prior_layout(ep["nodes"], pchunk, moves=sizes)[1]
    assert 3 <= P_reclaim < P
    assert arena_peak(eng)[0] == P_reclaim
    eng.check(); eng.close()
    eng, sizes = play(P_reclaim * pchunk)
    assert sizes == ep["moves_at"] and arena_peak(eng)[0] == P_reclaim
    eng.check(); eng.close()
    with pytest.raises(L.EngineError) as ei:
        play((P_reclaim - 1) * pchunk)
    assert_capacity(ei.value, PRIOR)


def test_visited_arena_peak_within_bounds_and_exact_cap():
    """The reported peak V lies within the model's bounds for the oracle's tree (the independent check), V chunks are enough and
    V - 1 are not (the search is deterministic: the figure the engine reports is necessary and sufficient)."""
    inst, sims = cc.SINGLE, cc.SMALL[3]
    ep = cc.auto_episode(inst, sims)
    caps = ample(inst)
    _, vchunk = chunk_sizes(inst)
    lo, hi = arena_ref.visited_bounds(ep["nodes"], vchunk)
    assert lo >= 3
    eng = play_single(inst, sims, **caps)
    run_until_idle(eng, evaluator(inst))
    assert_single_matches(eng, ep)
    V = arena_peak(eng)[1]
    eng.close()
    assert lo <= V <= hi, (lo, V, hi)
    eng = play_single(inst, sims, **dict(caps, vis_cap=V * vchunk))
    run_until_idle(eng, evaluator(inst))
    assert_single_matches(eng, ep)
    assert arena_peak(eng)[1] == V
    eng.close()
    eng = play_single(inst, sims, **dict(caps, vis_cap=(V - 1) * vchunk))
    assert_single_overflows(eng, inst, VISITED)
    eng.close()


@pytest.mark.parametrize("arena", [NODE, PRIOR, VISITED])
def test_a_starved_slot_fails_alone_and_recovers(arena):
    """Five slots, the neediest instance in slot 2, the cap set so that only it overflows (node caps from the oracle, chunk caps from
    the model).  One error, naming the arena; slot 2 is RP_PHASE_FAILED; the other four finish with the oracle's actions, outcomes,
    scores and complete trees.  Then rp_begin_episodes on all five slots with instances that fit: all five equal the oracle."""
    L = lib()
    sims = cc.SMALL[3]
    insts = cc.ISOLATION
    W, H, N = insts[0][:3]
    eps = [cc.auto_episode(i, sims) for i in insts]
    others = [k for k in range(5) if k != cc.NEEDIEST]
    caps = ample(insts[0])
    pchunk, vchunk = chunk_sizes(insts[0])
    if arena == NODE:
        caps["node_cap"] = max(eps[k]["n_nodes"] for k in others)
        assert eps[cc.NEEDIEST]["n_nodes"] > caps["node_cap"]
    elif arena == PRIOR:
        need = [arena_ref.prior_layout(e["nodes"], pchunk)[1] for e in eps]
        caps["edge_cap"] = max(need[k] for k in others) * pchunk
        assert need[cc.NEEDIEST] * pchunk > caps["edge_cap"]
    else:
        bounds = [arena_ref.visited_bounds(e["nodes"], vchunk) for e in eps]
        caps["vis_cap"] = max(bounds[k][1] for k in others) * vchunk
        assert bounds[cc.NEEDIEST][0] * vchunk > caps["vis_cap"]
    eng = make_engine(insts[0], 5, sims, **caps)
    eng.set_trace(True)
    area = np.full(5, W * H, np.int32)
    eng.begin_episodes(np.stack([e["wh"] for e in eps]), area, episode_id=100 + np.arange(5))
    errors = run_collecting_errors(eng, evaluator(insts[0]))
    assert len(errors) == 1
    assert_capacity(errors[0], arena)
    eng.check()  # reported once
    want = [L.PHASE_EPISODE_DONE] * 5
    want[cc.NEEDIEST] = L.PHASE_FAILED
    assert eng.status()[0].tolist() == want
    assert_records(eng, {100 + k: eps[k] for k in others})
    for k in others:
        assert_slot_equals_oracle(eng, k, eps[k], "slot %d next to the starved one" % k)
    # recovery
    fit = [eps[k] for k in cc.RECOVERY]
    eng.begin_episodes(np.stack([e["wh"] for e in fit]), area, episode_id=200 + np.arange(5))
    run_until_idle(eng, evaluator(insts[0]))
    eng.check()
    assert eng.status()[0].tolist() == [L.PHASE_EPISODE_DONE] * 5
    assert_records(eng, {200 + k: fit[k] for k in range(5)})
    for k in range(5):
        assert_slot_equals_oracle(eng, k, fit[k], "slot %d after the restart" % k)
    eng.check()
    # the same failure again, this time restarted by rp_begin_pool: each slot draws one instance of a pool of five that fit
    eng.begin_episodes(np.stack([e["wh"] for e in eps]), area, episode_id=300 + np.arange(5))
    errors = run_collecting_errors(eng, evaluator(insts[0]))
    assert len(errors) == 1
    assert_capacity(errors[0], arena)
    assert eng.status()[0].tolist() == want
    assert_records(eng, {300 + k: eps[k] for k in others})
    eng.set_instance_pool(np.stack([e["wh"] for e in fit]), area, first_id=400)
    eng.begin_pool()
    run_until_idle(eng, evaluator(insts[0]))
    eng.check()
    ph, _, _, episode = eng.status()
    assert ph.tolist() == [L.PHASE_EPISODE_DONE] * 5 and sorted(int(i) for i in episode) == list(range(400, 405))
    assert_records(eng, {400 + k: fit[k] for k in range(5)})
    for k in range(5):
        assert_slot_equals_oracle(eng, k, fit[int(episode[k]) - 400], "slot %d after the pool's restart" % k)
    eng.check()
    eng.close()


def test_illegal_external_action_fails_its_slot_only():
    """rp_advance_roots with a legal action in slots 0 and 2 and, in slot 1, an action of an item that is already placed:
    RP_ERR_ASSERT, slot 1 is RP_PHASE_FAILED, slots 0 and 2 have moved exactly as the oracle moves."""
    L = lib()
    sims = cc.SMALL[3]
    insts = cc.ISOLATION[:3]
    W, H, N = insts[0][:3]
    whs = [cc.items_of(i) for i in insts]
    eng = make_engine(insts[0], 3, sims, rule=L.MOVE_EXTERNAL)
    eng.begin_episodes(np.stack(whs), np.full(3, W * H, np.int32))
    ms, boards, rems = [], [], []
    for wh in whs:
        m = cc.new_oracle(W, H, N)
        m.begin_episode(wh[:, 0], wh[:, 1], W * H, cc.BUF)
        ms.append(m); boards.append(np.zeros((H, W), np.uint8)); rems.append(np.ones(N, np.uint8))

    def search_and_pick(slots):
        run_until_idle(eng, evaluator(insts[0]))
        counts = eng.root_counts()
        acts = {}
        for g in slots:
            want = ms[g].action_counts(boards[g], rems[g], sims)
            assert np.array_equal(counts[g], want), g
            acts[g] = int(np.argmax(want))
        return acts

    def oracle_moves(acts):
        for g, a in acts.items():
            _, boards[g], rems[g] = orc.next_state(W, H, N, boards[g], whs[g][:, 0], whs[g][:, 1], rems[g], a)

    first = search_and_pick(range(3))
    ended, _ = eng.advance_roots([first[g] for g in range(3)])
    assert ended.tolist() == [0, 0, 0]
    oracle_moves(first)
    second = search_and_pick(range(3))
    placed = first[1] // W
    assert rems[1][placed] == 0
    with pytest.raises(L.EngineError) as ei:
        eng.advance_roots([second[0], placed * W, second[2]])
    assert ei.value.code == L.ERR_ASSERT and "not a legal move" in str(ei.value)
    eng.check()
    ph, _, moves, _ = eng.status()
    assert ph.tolist() == [L.PHASE_RUNNING, L.PHASE_FAILED, L.PHASE_RUNNING] and moves.tolist() == [2, 1, 2]
    oracle_moves({0: second[0], 2: second[2]})
    search_and_pick((0, 2))
    for g in (0, 2):
        d = eng.dump_tree(g)
        dump = ms[g].dump()
        assert_trees_equal(tree_as_dict(d), dump, "slot %d" % g)
        assert engine_keys(d) == list(dump.keys())
    eng.check()
    eng.close()
    for m in ms:
        m.close()


@pytest.mark.parametrize("trace", [False, True], ids=["records", "packings"])
def test_finished_ring_overflow_keeps_the_first_records(trace):
    """16 slots restart through a pool of fin_cap + 6 instances and nothing is popped: RP_ERR_CAPACITY naming the ring, the ring holds
    exactly fin_cap records with distinct ids of the pool, each the oracle's result for its instance (with the trace: its packing
    too).  A second pool is then popped whole and correct."""
    W, H, N, sims = cc.TINY
    inst = (W, H, N, H, 0)
    G, fin_cap, pool = cc.RING_SLOTS, cc.RING_CAP, cc.RING_POOL
    eps = cc.tiny_episodes()
    eng = make_engine(inst, G, sims, auto_restart=1)
    eng.set_trace(trace)
    wh = np.stack([eps[k % len(eps)]["wh"] for k in range(pool)])
    eng.set_instance_pool(wh, np.full(pool, W * H, np.int32), first_id=5000)
    eng.begin_pool()
    errors = run_collecting_errors(eng, evaluator(inst))
    assert 1 <= len(errors) <= pool - fin_cap  # every record that found no room reports, launches apart
    for e in errors:
        assert_capacity(e, RING)
    eng.check()
    assert (eng.status()[0] == lib().PHASE_IDLE).all()
    rec = eng.pop_finished(packings=True) if trace else eng.pop_finished()
    ids = [int(i) for i in rec[0]]
    assert len(ids) == fin_cap and len(set(ids)) == fin_cap and min(ids) >= 5000 and max(ids) < 5000 + pool
    for k, i in enumerate(ids):
        ep = eps[(i - 5000) % len(eps)]
        n = len(ep["actions"])
        assert (int(rec[1][k]), float(rec[2][k]), int(rec[3][k])) == (ep["outcome"], ep["score"], n), i
        if trace:
            assert rec[4][k].tolist() == ep["actions"] + [0] * (N - n) and [int(x) for x in rec[5][k]] == ep["filled"] + [0] * (N - n), i
            assert np.array_equal(rec[6][k], ep["board"]), i
    assert len(eng.pop_finished()[0]) == 0
    eng.set_instance_pool(wh[3:23], np.full(20, W * H, np.int32), first_id=9000)
    eng.begin_pool()
    run_until_idle(eng, evaluator(inst))
    eng.check()
    assert_records(eng, {9000 + k: eps[(3 + k) % len(eps)] for k in range(20)}, trace)
    eng.close()


def _replay_engine(games, onehot, **kw):
    inst = cc.REPLAY_POOL[0]
    eng = make_engine(inst, games, cc.REPLAY_SIMS, auto_restart=1, **kw)
    if onehot:
        eng.set_move_rule(lib().MOVE_ARGMAX_FIRST, onehot_examples=True)
    return eng


def _run_replay_pool(eng, insts, first_id):
    """-> (errors, {episode id: outcome} of the pool)."""
    W, H, N = insts[0][:3]
    eng.set_instance_pool(np.stack([cc.items_of(i) for i in insts]), np.full(len(insts), W * H, np.int32), first_id=first_id)
    eng.begin_pool()
    errors = run_collecting_errors(eng, evaluator(insts[0]))
    ids, outcome, _, moves = eng.pop_finished()
    assert sorted(int(i) for i in ids) == list(range(first_id, first_id + len(insts)))
    return errors, {int(i): (int(o), int(m)) for i, o, m in zip(ids, outcome, moves)}


def _examples(eng):
    """The packed replay buffer -> (E, S, {(episode, move): (key bytes, item sizes bytes, value, sorted (action, count) pairs)})."""
    t = {k: v.cpu().numpy() for k, v in eng.examples_packed("cuda").items()}
    E, S = len(t["value"]), len(t["sp_act"])
    out = {}
    for k in range(E):
        lo, n = int(t["sp_off"][k]), int(t["sp_n"][k])
        assert 0 <= lo and lo + n <= S
        pairs = sorted(zip((t["sp_act"][lo:lo + n].astype(np.int64) & 0xFFFF).tolist(), t["sp_cnt"][lo:lo + n].tolist()))
        key = (int(t["episode"][k]), int(t["move"][k]))
        assert key not in out
        out[key] = (t["key"][k].tobytes(), t["wh"][k].tobytes(), int(t["value"][k]), tuple(pairs))
    return E, S, out


def _assert_values_are_own_outcomes(ex, fin):
    """Every kept example carries the outcome of ITS episode -- not of an episode that ended later in the same slot."""
    for (episode, move), rec in ex.items():
        assert rec[2] == fin[episode][0] and 0 <= move < fin[episode][1], (episode, move, rec[2], fin[episode])


def test_replay_buffer_example_cap_exact_and_one_short():
    """max_examples = the pool's moves (from the oracle): clean and full.  One fewer: RP_ERR_CAPACITY naming the replay buffer, the
    examples that fitted are intact and every one of them has its own episode's outcome; after rp_examples_clear the engine records
    another pool exactly like an engine that never overflowed."""
    pool = cc.REPLAY_POOL
    eps = [cc.auto_episode(i, cc.REPLAY_SIMS) for i in pool]
    total = sum(len(e["actions"]) for e in eps)
    ref = _replay_engine(1, False, max_examples=total)
    errors, fin = _run_replay_pool(ref, pool, 300)
    assert errors == []
    E, S, ex1 = _examples(ref)
    assert E == total == len(ex1)
    _assert_values_are_own_outcomes(ex1, fin)
    for k, ep in enumerate(eps):  # the recorded visit counts are the oracle's
        assert fin[300 + k] == (ep["outcome"], len(ep["actions"]))
        for mv in range(len(ep["actions"])):
            c = ep["counts"][mv]
            assert ex1[(300 + k, mv)][3] == tuple((int(a), int(c[a])) for a in np.nonzero(c)[0]), (k, mv)
    ref.examples_clear()
    errors, fin2 = _run_replay_pool(ref, pool[:-1], 700)
    assert errors == []
    E2, S2, ex2 = _examples(ref)
    assert E2 == total - len(eps[-1]["actions"])
    _assert_values_are_own_outcomes(ex2, fin2)
    ref.check(); ref.close()

    short = _replay_engine(1, False, max_examples=total - 1)
    errors, fin = _run_replay_pool(short, pool, 300)
    assert len(errors) == 1
    assert_capacity(errors[0], REPLAY)
    short.check()
    E, S, ex = _examples(short)
    assert E == total - 1 == len(ex)
    _assert_values_are_own_outcomes(ex, fin)  # decides the stale-index question: an entry of slot_ex this episode did not set
    assert all(ex1[k] == v for k, v in ex.items())
    short.examples_clear()
    errors, fin2s = _run_replay_pool(short, pool[:-1], 700)
    assert errors == [] and fin2s == fin2
    assert _examples(short) == (E2, S2, ex2)
    short.check(); short.close()


def test_replay_buffer_pair_cap_exact_and_one_short():
    """The same for max_sparse, with one-hot examples so that the pairs are one per example, and three slots filling the buffer
    concurrently.  One pair too few: the example whose pair did not fit is kept without pairs, nothing else changes."""
    pool = cc.REPLAY_POOL
    eps = [cc.auto_episode(i, cc.REPLAY_SIMS) for i in pool]
    total = sum(len(e["actions"]) for e in eps)
    ref = _replay_engine(3, True, max_examples=total + 8, max_sparse=total)
    errors, fin = _run_replay_pool(ref, pool, 300)
    assert errors == []
    E, S, ex1 = _examples(ref)
    assert (E, S) == (total, total)
    _assert_values_are_own_outcomes(ex1, fin)
    for k, ep in enumerate(eps):
        for mv, a in enumerate(ep["actions"]):
            assert ex1[(300 + k, mv)][3] == ((a, 1),), (k, mv)
    ref.examples_clear()
    errors, fin2 = _run_replay_pool(ref, pool[:-1], 700)
    assert errors == []
    E2, S2, ex2 = _examples(ref)
    ref.check(); ref.close()

    short = _replay_engine(3, True, max_examples=total + 8, max_sparse=total - 1)
    errors, fin = _run_replay_pool(short, pool, 300)
    assert len(errors) == 1
    assert_capacity(errors[0], REPLAY)
    short.check()
    E, S, ex = _examples(short)
    assert (E, S) == (total, total - 1)
    _assert_values_are_own_outcomes(ex, fin)
    lost = [k for k, v in ex.items() if v[3] == ()]
    assert len(lost) == 1
    assert all(v == ex1[k] or (k in lost and v[:3] == ex1[k][:3]) for k, v in ex.items())
    short.examples_clear()
    errors, fin2s = _run_replay_pool(short, pool[:-1], 700)
    assert errors == [] and fin2s == fin2
    assert _examples(short) == (E2, S2, ex2)
    short.check(); short.close()
