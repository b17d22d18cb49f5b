"""GPU parity of the incumbents (rp_set_incumbent / rp_pop_finished_best / rp_incumbents, BatchedSelfPlay's record_best, solve.pack's
best=True) against the incumbent read out of the CPU oracle's tree (tests/best_ref.py).  Every comparison is exact: integers, and
doubles produced by the same arithmetic."""
import numpy as np
import pytest

import best_ref as br
import evaluators as ev
import initial_ref as ir
import oracle_lib as orc
from engine_util import host_evaluator, run_until_idle

pytestmark = pytest.mark.gpu
FIELDS = ("score", "outcome", "moves", "prefix", "updates", "action", "board")


def kind_of_slot(s):
    return br.KINDS[s % 2]


def table_evaluator(W, N):
    return host_evaluator(kind_of_slot, W * N, lambda s: br.SALT)


def make_engine(W, H, N, games, sims, rule, **kw):
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=br.ALPHA, move_rule=rule, seed=br.SEED, tie_salt=br.SALT, **kw)
    eng.set_rank_buffer(br.BUF)
    return eng


def best_records(eng, packings=False):
    """-> {episode id: dict(outcome, score, moves, best fields ..., [played action list])}"""
    rec = eng.pop_finished(packings=packings, best=True)
    ids, oc, sc, mv, best = rec[0], rec[1], rec[2], rec[3], rec[-1]
    assert len(set(ids.tolist())) == len(ids), "an episode was recorded twice"
    out = {}
    for k, i in enumerate(ids):
        out[int(i)] = dict(p_outcome=int(oc[k]), p_score=float(sc[k]), p_moves=int(mv[k]), **{f: best[f][k] for f in FIELDS})
        if packings:
            out[int(i)]["p_action"] = [int(a) for a in rec[4][k, :int(mv[k])]]
    return out


def check_best(got, ref, W, H, N, wh, played, where, initial_rows=None, initial_rem=None):
    """One finished record (or running incumbent) against best_ref."""
    m = int(got["moves"])
    assert float(got["score"]) == ref["score"], (where, float(got["score"]), ref["score"])
    assert int(got["outcome"]) == ref["outcome"], where
    assert np.array_equal(got["board"], ref["rows"]), where
    assert m == int((np.ones(N, np.uint8) if initial_rem is None else (np.asarray(initial_rem) != 0)).sum()) - int(ref["rem"].sum()), where
    assert int(got["updates"]) == ref["updates"], (where, int(got["updates"]), ref["updates"])
    assert not got["action"][m:].any(), where  # zero past the incumbent's moves
    assert 0 <= int(got["prefix"]) <= m
    br.check_actions(ref, W, H, N, wh, got["action"][:m], int(got["prefix"]), played, initial_rows, initial_rem, where)


def play_and_check(W, H, bin_h, N, sims, games, rule, policy, **engine_kw):
    wh = br.instances(W, bin_h, N, games)
    eng = make_engine(W, H, N, games, sims, rule, **engine_kw)
    eng.set_trace(True)
    eng.set_incumbent(True)
    eng.begin_episodes(wh, np.full(games, W * bin_h, np.int32), episode_id=np.arange(games))
    run_until_idle(eng, table_evaluator(W, N))
    got = best_records(eng, packings=True)
    assert sorted(got) == list(range(games))
    better = 0
    for g in range(games):
        played, outcome, score, ref = br.oracle_episode(W, H, N, wh[g], W * bin_h, br.BUF, kind_of_slot(g), sims, policy, br.SEED, g)
        rec = got[g]
        assert (rec["p_action"], rec["p_outcome"], rec["p_score"]) == (played, outcome, score), g  # the trace is what it was
        check_best(rec, ref, W, H, N, wh[g], played, "game %d" % g)
        assert float(rec["score"]) >= rec["p_score"]
        better += float(rec["score"]) > rec["p_score"]
    eng.close()
    return better


# ---- 1. / 2. oracle parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["sample", "argmax_first"])
@pytest.mark.parametrize("W,H,bin_h,N,sims,games", [(10, 10, 5, 8, 10, 8), (6, 8, 4, 5, 12, 8), (15, 15, 9, 10, 30, 6)])
def test_incumbent_matches_the_oracle(rule, W, H, bin_h, N, sims, games):
    from resource_packing_self_play_amd import _lib
    rule, policy = dict(sample=(_lib.MOVE_SAMPLE, br.SAMPLE), argmax_first=(_lib.MOVE_ARGMAX_FIRST, br.ARGMAX_FIRST))[rule]
    play_and_check(W, H, bin_h, N, sims, games, rule, policy)


def test_incumbent_matches_the_oracle_on_64_bit_rows():
    from resource_packing_self_play_amd import _lib
    play_and_check(40, 6, 3, 6, 12, 2, _lib.MOVE_SAMPLE, br.SAMPLE)


# ---- 3. the second path register pair: depth > 64 ------------------------------------------------------------------------------------------
def test_incumbent_of_a_path_deeper_than_64():
    """72 small items and an evaluator that is one-hot on the lowest legal action: every simulation goes one level deeper along one
    line, and within 80 simulations from the initial root the tree holds terminals at level 72.  No move is played."""
    from resource_packing_self_play_amd import _lib
    W, H, N, sims = 8, 12, 72, 80
    wh = np.array([[2 if k % 5 == 4 else 1, 1] for k in range(N)], np.uint8)
    area = int((wh[:, 0].astype(np.int64) * wh[:, 1]).sum())

    def lowest_legal(board, rem):
        valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        pi = np.zeros(W * N, np.float32)
        pi[int(np.flatnonzero(valid)[0])] = 1.0
        return pi, np.zeros(1, np.float32)

    def evaluate(rows, rem, slots):
        out = [lowest_legal(ev.unpack_board(rows[b], W), rem[b]) for b in range(len(rows))]
        return np.stack([p for p, _ in out]), np.array([v[0] for _, v in out], np.float32)

    m = orc.OracleMCTS(W, H, N, 1.0, br.ALPHA, lowest_legal, lambda b, r: ev.tie_value(ev.pack_board(b), r, br.SALT))
    m.begin_episode(wh[:, 0], wh[:, 1], area, br.BUF)
    m.action_counts(np.zeros((H, W), np.uint8), np.ones(N, np.uint8), sims)
    ref = br.best_of_dump(m.dump(), W, H, area, 1, br.BUF)
    m.close()
    assert int(ref["rem"].sum()) == 0, "the oracle's tree holds no terminal at level 72"

    eng = make_engine(W, H, N, 1, sims, _lib.MOVE_EXTERNAL)
    eng.set_incumbent(True)
    eng.begin_episodes(wh[None], [area], episode_id=[0])
    none_yet = eng.incumbents()
    assert none_yet["moves"][0] == -1 and none_yet["updates"][0] == 0 and not none_yet["action"].any() and not none_yet["board"].any()
    run_until_idle(eng, evaluate)
    inc = eng.incumbents()
    got = {f: inc[f][0] for f in FIELDS}
    assert int(got["moves"]) == 72 and int(got["prefix"]) == 0
    check_best(got, ref, W, H, N, wh, [], "deep path")
    eng.close()


# ---- 4. pool and reset ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reclaim", [0, 1])
def test_pool_episodes_keep_their_own_incumbent(reclaim):
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, slots, n_inst, first_id = 10, 10, 5, 8, 10, 3, 8, 70
    wh = br.instances(W, bin_h, N, n_inst)
    eng = make_engine(W, H, N, slots, sims, _lib.MOVE_SAMPLE, auto_restart=1, reclaim=reclaim)
    eng.set_incumbent(True)  # the trace stays off: the two do not need each other
    eng.set_instance_pool(wh, np.full(n_inst, W * bin_h, np.int32), first_id)
    eng.begin_pool()
    run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: br.SALT))  # episodes change slots: one evaluator for all
    got = best_records(eng)
    assert sorted(got) == list(range(first_id, first_id + n_inst))
    for k in range(n_inst):
        played, outcome, score, ref = br.oracle_episode(W, H, N, wh[k], W * bin_h, br.BUF, "hashed", sims, br.SAMPLE, br.SEED, first_id + k)
        rec = got[first_id + k]
        assert (rec["p_outcome"], rec["p_score"], rec["p_moves"]) == (outcome, score, len(played)), k
        check_best(rec, ref, W, H, N, wh[k], played, "instance %d" % k)
    eng.close()


# ---- 5. starts ------------------------------------------------------------------------------------------------------------------------
def test_incumbents_of_initial_states():
    """A pool of three: an instance whose initial state is terminal (a full bin), one started in the middle of a packing, and the plain
    start as the control."""
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, first_id = 10, 10, 5, 8, 12, 20
    wh = br.instances(W, bin_h, N, 3)
    boards, rems, areas = [], [], []
    boards.append(np.ones((H, W), np.uint8)); rems.append(np.ones(N, np.uint8)); areas.append(W * H)  # nothing fits: an episode of 0 moves
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    for _ in range(3):  # three legal moves into the packing
        valid, n = orc.valid_moves(W, H, N, board, wh[1][:, 0], wh[1][:, 1], rem)
        rc, board, rem = orc.next_state(W, H, N, board, wh[1][:, 0], wh[1][:, 1], rem, int(np.flatnonzero(valid)[-1]))
    boards.append(board); rems.append(rem); areas.append(W * bin_h)
    boards.append(np.zeros((H, W), np.uint8)); rems.append(np.ones(N, np.uint8)); areas.append(W * bin_h)
    rows = np.stack([ev.pack_board(b) for b in boards])
    eng = make_engine(W, H, N, 2, sims, _lib.MOVE_SAMPLE, auto_restart=1)
    eng.set_incumbent(True)
    eng.set_instance_pool(wh, np.array(areas, np.int32), first_id)
    eng.set_instance_initial(rows, np.stack(rems))
    eng.begin_pool()
    run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: br.SALT))
    got = best_records(eng)
    assert sorted(got) == [first_id, first_id + 1, first_id + 2]
    for k in range(3):
        m = br.new_oracle(W, H, N, "hashed")
        ir.begin(m, wh[k], rems[k], areas[k], br.BUF, br.SALT)
        want = ir.play_from(m, boards[k], rems[k], sims, ir.SAMPLE, br.SEED, first_id + k)
        ref = br.best_of_dump(m.dump(), W, H, areas[k], m.episode["max_h"], br.BUF) if want["moves"] else None
        sizes = np.stack([m.episode["iw"], m.episode["ih"]], axis=1)
        m.close()
        rec = got[first_id + k]
        assert (rec["p_outcome"], rec["p_score"], rec["p_moves"]) == (want["outcome"], want["score"], want["moves"]), k
        if k == 0:  # the oracle never builds a tree for it: the incumbent is the initial state itself
            assert want["moves"] == 0 and int(rec["moves"]) == 0 and int(rec["prefix"]) == 0 and int(rec["updates"]) == 1
            assert np.array_equal(rec["board"], rows[0]) and not rec["action"].any()
            assert (float(rec["score"]), int(rec["outcome"])) == (want["score"], want["outcome"])
        else:
            check_best(rec, ref, W, H, N, sizes, want["actions"], "instance %d" % k, rows[k], rems[k])
            assert float(rec["score"]) >= rec["p_score"]
    eng.close()


# ---- 6. external moves the search never tried -----------------------------------------------------------------------------------------------
def test_external_moves_without_a_search():
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N = 10, 10, 5, 8
    wh = br.instances(W, bin_h, N, 1)[0]
    board, rem, seq = np.zeros((H, W), np.uint8), np.ones(N, np.uint8), []
    while True:  # a fixed legal sequence: always the highest legal action
        valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        if n == 0:
            break
        seq.append(int(np.flatnonzero(valid)[-1]))
        rc, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, seq[-1])
    _, r = orc.ranked_reward(W, H, board, W * bin_h, int(wh[:, 1].max()), br.BUF, br.ALPHA)
    eng = make_engine(W, H, N, 1, 0, _lib.MOVE_EXTERNAL, node_cap=N + 2)  # the automatic arena is sized by sims: room for the line itself
    eng.set_incumbent(True)
    eng.begin_episodes(wh[None], [W * bin_h], episode_id=[9])
    for k, a in enumerate(seq):
        assert eng.incumbents()["moves"][0] == -1  # nothing terminal yet
        ended, score = eng.advance_roots([a])
        assert (ended[0] != 0) == (k + 1 == len(seq))
    rec = best_records(eng)[9]
    m = len(seq)
    assert int(rec["moves"]) == m == rec["p_moves"] and int(rec["prefix"]) == m - 1 and int(rec["updates"]) == 1
    assert [int(a) for a in rec["action"][:m]] == seq and not rec["action"][m:].any()
    assert np.array_equal(rec["board"], ev.pack_board(board))
    assert float(rec["score"]) == r == rec["p_score"] and int(rec["outcome"]) == rec["p_outcome"]
    eng.close()


# ---- 7. scheduling changes nothing ----------------------------------------------------------------------------------------------------
def test_step_cap_and_compact_rows_change_nothing():
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, games = 10, 10, 5, 8, 10, 8
    wh = br.instances(W, bin_h, N, games)
    runs = []
    for cap, compact in ((0, False), (1, False), (0, True), (1, True)):
        eng = make_engine(W, H, N, games, sims, _lib.MOVE_SAMPLE)
        eng.set_step_cap(cap)
        eng.set_compact_rows(compact)
        eng.set_incumbent(True)
        eng.begin_episodes(wh, np.full(games, W * bin_h, np.int32), episode_id=np.arange(games))
        run_until_idle(eng, table_evaluator(W, N))
        runs.append(best_records(eng))
        eng.close()
    for other in runs[1:]:
        assert sorted(other) == sorted(runs[0])
        for g, rec in runs[0].items():
            for f, val in rec.items():
                assert np.array_equal(val, other[g][f]), (g, f)


def test_graph_replay_and_the_switch_change_nothing():
    """The seeded CNN in the loop: HIP graphs against eager waves with record_best on, and record_best off against on."""
    import torch
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    from test_gpu_packings import cnn_setup
    W, H, N, sims, games = 10, 10, 8, 20, 16
    game, nnet, args = cnn_setup(W, H, N, sims)
    wh = br.instances(W, 6, N, games)
    area = np.full(games, W * 6, np.int32)
    runs = {}
    for graph, best in ((True, True), (False, True), (True, False)):
        sp = BatchedSelfPlay(game, nnet, args, games=games, move_rule=_lib.MOVE_SAMPLE, seed=77, groups=2, max_examples=games * N, use_graph=graph,
                             tie_salt=3, record_packings=True, record_best=best)
        ids, outcome, score, moves, _ = sp.run(wh, area, br.BUF, first_id=500)
        rep = sp.examples_packed()
        planes, pi, value = rep.dense()
        runs[(graph, best)] = dict(result=(ids, outcome, score, moves), packs=sp.pop_packings(), best=sp.pop_best_packings(),
                                   examples=[t.cpu().numpy() for t in (rep.key, rep.episode, rep.move, planes, pi, value)])
        sp.close()
    a, b, off = runs[(True, True)], runs[(False, True)], runs[(True, False)]
    assert [p.episode_id for p in a["best"]] == list(range(500, 500 + games)) and off["best"] == []
    for p, q, played in zip(a["best"], b["best"], a["packs"]):
        assert p == q and (p.prefix, p.updates) == (q.prefix, q.updates)  # identical in every field
        assert p.score >= played.score and p.actions[:p.prefix].tolist() == played.actions[:p.prefix].tolist()
        p.layout()
    for on in (a, b):  # the switch changes nothing it does not add
        assert on["packs"] == off["packs"]
        for x, y in zip(on["result"] + tuple(on["examples"]), off["result"] + tuple(off["examples"])):
            assert np.array_equal(x, y)
    torch.cuda.synchronize()


# ---- 8. cost and refusals -------------------------------------------------------------------------------------------------------------
def test_cost_and_refusals():
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, games = 10, 10, 5, 8, 10, 5
    wh = br.instances(W, bin_h, N, games)
    eng = make_engine(W, H, N, games, sims, _lib.MOVE_ARGMAX_FIRST)
    off = eng.device_bytes
    with pytest.raises(_lib.EngineError) as ei:  # incumbents off
        eng.pop_finished(best=True)
    assert ei.value.code == _lib.ERR_ARG and "incumbent" in str(ei.value)
    with pytest.raises(_lib.EngineError) as ei:
        eng.incumbents()
    assert ei.value.code == _lib.ERR_ARG
    eng.set_incumbent(False)
    assert eng.device_bytes == off  # nothing before the first enable
    eng.set_incumbent(True)
    stride = (24 + 8 * H + 4 * N + 7) // 8 * 8
    assert eng.device_bytes - off == (games + max(4 * games, 1024)) * stride + 16 * games  # the cost rp_engine.h documents
    eng.set_incumbent(True)
    assert eng.device_bytes - off == (games + max(4 * games, 1024)) * stride + 16 * games  # allocated once
    eng.begin_episodes(wh, np.full(games, W * bin_h, np.int32))
    for on in (False, True):  # refused while episodes are being played, in either direction
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_incumbent(on)
        assert ei.value.code == _lib.ERR_STATE
    with pytest.raises(_lib.EngineError) as ei:  # re-rooting: the moves to the new root are unknown
        eng.set_roots(np.zeros((1, H), np.uint64), np.ones((1, N), np.uint8))
    assert ei.value.code == _lib.ERR_STATE and "incumbent" in str(ei.value)
    run_until_idle(eng, table_evaluator(W, N))
    with pytest.raises(_lib.EngineError) as ei:  # a trace output while the trace is off
        eng.pop_finished(packings=True, best=True)
    assert ei.value.code == _lib.ERR_ARG and "trace" in str(ei.value)
    assert len(eng.pop_finished(max_n=2, best=True)[0]) == 2  # one ring, one cursor
    assert len(eng.pop_finished(max_n=1)[0]) == 1
    assert len(eng.pop_finished(best=True)[0]) == games - 3
    eng.set_incumbent(False)
    eng.set_roots(np.zeros((1, H), np.uint64), np.ones((1, N), np.uint8))  # allowed again
    eng.close()


# ---- 9. the public API ----------------------------------------------------------------------------------------------------------------
def check_public(best, wh, n):
    assert [p.episode_id for p in best] == list(range(n))
    for k, p in enumerate(best):
        p.layout(); p.played.layout()
        assert np.array_equal(p.item_wh, wh[k]) and p.played.episode_id == k
        assert p.score >= p.played.score and p.updates >= 1 and 0 <= p.prefix <= p.moves
        assert p.actions[:p.prefix].tolist() == p.played.actions[:p.prefix].tolist()
        assert p.played.prefix is None and p.played.played is None


def test_pack_returns_the_incumbents():
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.solve import pack, random_scores
    from test_gpu_packings import cnn_setup
    W, H, bin_h, N, sims, games = 10, 10, 5, 8, 10, 8
    wh = br.instances(W, bin_h, N, games)
    area = np.full(games, W * bin_h, np.int32)
    game, nnet, args = cnn_setup(W, H, N, sims)
    best = pack(game, nnet, args, item_wh=wh, total_area=area, rewards_list=br.BUF, move_rule=_lib.MOVE_SAMPLE, best=True)
    check_public(best, wh, games)
    played = pack(game, nnet, args, item_wh=wh, total_area=area, rewards_list=br.BUF, move_rule=_lib.MOVE_SAMPLE)  # the default path: unchanged
    assert played == [p.played for p in best] and all(p.prefix is None for p in played)
    buf = random_scores(game, item_wh=wh, playouts=4, seed=1).ravel()
    best = pack(game, None, args, item_wh=wh, total_area=area, rewards_list=buf, move_rule=_lib.MOVE_SAMPLE, evaluator="rollout", playouts=4, best=True)
    check_public(best, wh, games)
