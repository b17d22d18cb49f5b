"""GPU parity of the move rule that follows the incumbent (RP_MOVE_INCUMBENT, include/rp_engine.h) against the rule restated over the CPU
oracle (tests/move_incumbent_ref.py), which knows every incumbent's action list: the comparisons are exact -- integers, lists, and doubles
produced by the same arithmetic.  tests/test_move_incumbent_cpu.py proves that the instances played here reach every branch of the rule."""
import ctypes as C
import functools

import numpy as np
import pytest

import best_playout_ref as bp
import best_ref as br
import move_incumbent_ref as mi
from engine_util import assert_trees_equal, host_evaluator, run_until_idle, tree_as_dict
from test_move_incumbent_cpu import SWITCHES

pytestmark = pytest.mark.gpu
PLAYOUTS = 3
SETTINGS = {"uniform": (mi.UNIFORM, 0), "width2+landing2": (mi.WIDTH2, 2)}  # playout policy (w_pow, h_pow), landing power


@functools.lru_cache(maxsize=None)
def table_refs(shape, switch_at=0):
    games = br.SHAPES[shape][5]
    return [mi.probe(shape, g, switch_at=switch_at, want_tree=True)[1] for g in range(games)]


@functools.lru_cache(maxsize=None)
def playout_refs(shape, setting):
    policy, land_pow = SETTINGS[setting]
    return [mi.probe(shape, g, playouts=PLAYOUTS, policy=policy, land_pow=land_pow, want_tree=True)[1] for g in range(br.SHAPES[shape][5])]


def table_evaluator(W, N, kind_of_slot=lambda s: br.KINDS[s % 2]):
    return host_evaluator(kind_of_slot, W * N, lambda s: br.SALT)


def follow_engine(W, H, N, games, sims, playouts=False, setting="uniform", onehot=False, **kw):
    """An engine under RP_MOVE_INCUMBENT: created with the rule's own fallback, the incumbents switched on, then the rule."""
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=br.ALPHA, move_rule=_lib.MOVE_ARGMAX_FIRST, seed=br.SEED, tie_salt=br.SALT,
                      stream=torch.cuda.current_stream().cuda_stream, **kw)
    eng.set_rank_buffer(br.BUF)
    eng.set_trace(True)
    eng.set_incumbent(True)
    if playouts:
        eng.set_incumbent_playouts(True)
        (w_pow, h_pow), land_pow = SETTINGS[setting]
        eng.set_playout_policy(w_pow, h_pow)
        eng.set_playout_landing(land_pow)
    eng.set_move_rule(_lib.MOVE_INCUMBENT, onehot_examples=onehot)
    return eng


def rollout_loop(eng, playouts=PLAYOUTS):
    from test_gpu_best_playout import eager_loop
    eager_loop(eng, playouts)


def finished(eng):
    """-> {episode id: dict(p_outcome, p_score, p_action, best fields ...)}"""
    rec = eng.pop_finished(packings=True, best=True)
    ids, oc, sc, mv, act, board, best = rec[0], rec[1], rec[2], rec[3], rec[4], rec[6], rec[-1]
    assert len(set(ids.tolist())) == len(ids), "an episode was recorded twice"
    return {int(i): dict(p_outcome=int(oc[k]), p_score=float(sc[k]), p_action=[int(a) for a in act[k, :int(mv[k])]], p_board=board[k],
                         **{f: best[f][k] for f in best}) for k, i in enumerate(ids)}


def check_incumbent(got, want, where, sources=False):
    """An incumbent record of the engine (finished or running) against a record of the reference: every field, the action list included.
    sources: playout incumbents are on, so the record must carry tree_moves and playout, and they are compared too."""
    if want is None:
        assert int(got["moves"]) == -1, where
        return
    m = int(got["moves"])
    assert float(got["score"]) == want["score"], (where, float(got["score"]), want["score"])
    assert (int(got["outcome"]), m, int(got["prefix"]), int(got["updates"])) == (want["outcome"], want["moves"], want["prefix"], want["updates"]), where
    assert np.array_equal(got["board"], want["rows"]), where
    assert [int(a) for a in got["action"][:m]] == want["actions"] and not got["action"][m:].any(), where
    assert ("tree_moves" in got and "playout" in got) == sources, where
    if sources:
        assert (int(got["tree_moves"]), int(got["playout"])) == (want["tree_moves"], want["playout"]), where


def check_episode(rec, ref, where, from_start=True, sources=False):
    assert (rec["p_action"], rec["p_outcome"], rec["p_score"]) == (ref["actions"], ref["outcome"], ref["score"]), where
    assert np.array_equal(rec["p_board"], ref["board"]), where
    check_incumbent(rec, ref["best"], where, sources)
    if from_start and float(rec["score"]) > 0:  # the invariant of the rule in force since the episode began, on the engine's own record
        m = int(rec["moves"])
        assert [int(a) for a in rec["action"][:m]] == rec["p_action"] and float(rec["score"]) == rec["p_score"], where
        assert int(rec["outcome"]) == rec["p_outcome"] and np.array_equal(rec["board"], rec["p_board"]), where


def check_all(eng, refs, where, from_start=True):
    got = finished(eng)
    assert sorted(got) == list(range(len(refs)))
    for g, ref in enumerate(refs):
        check_episode(got[g], ref, "%s game %d" % (where, g), from_start, eng.incumbent_playouts)
        assert_trees_equal(tree_as_dict(eng.dump_tree(g)), ref["tree"], "%s game %d" % (where, g))
    cnt = eng.counters()
    assert cnt["followed_moves"] == sum(r["n_followed"] for r in refs) and cnt["moves"] == sum(len(r["actions"]) for r in refs), where


# ---- 1. tree terminals, host table evaluators ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", range(len(br.SHAPES)))
def test_tree_terminals_match_the_reference(shape):
    W, H, bin_h, N, sims, games = br.SHAPES[shape]
    eng = follow_engine(W, H, N, games, sims)
    eng.begin_episodes(br.instances(W, bin_h, N, games), np.full(games, W * bin_h, np.int32), episode_id=np.arange(games))
    run_until_idle(eng, table_evaluator(W, N))
    check_all(eng, table_refs(shape), "shape %d" % shape)
    eng.close()


# ---- 2. playouts as candidates --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", [1, 4])
def test_playout_incumbents_match_the_reference(shape, setting):
    """The followed tail of a playout incumbent is the playout's own moves, replayed under the setting that scored it."""
    W, H, bin_h, N, sims, games = br.SHAPES[shape]
    eng = follow_engine(W, H, N, games, sims, playouts=True, setting=setting)
    eng.begin_episodes(br.instances(W, bin_h, N, games), np.full(games, W * bin_h, np.int32), episode_id=np.arange(games))
    rollout_loop(eng)
    refs = playout_refs(shape, setting)
    assert any(r["best"]["playout"] >= 0 and r["followed"][-1] for r in refs)
    check_all(eng, refs, "shape %d %s" % (shape, setting))
    eng.close()


# ---- 3. the production route ------------------------------------------------------------------------------------------------------------------
def rollout_game(W, H, N, sims):
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(dict(numMCTSSims=sims, cpuct=1, alpha=br.ALPHA, cuda=True, num_items=N, num_bins=1))


def check_followed_packings(best, n):
    assert [p.episode_id for p in best] == list(range(n))
    for p in best:
        p.layout(); p.played.layout()
        if p.score > 0:
            assert p.score == p.played.score and p.actions.tolist() == p.played.actions.tolist() and p.outcome == p.played.outcome
            assert np.array_equal(p.board, p.played.board)
        else:
            assert p.played.score == 0


def test_graphs_groups_and_restarts_change_nothing():
    """Two groups, captured graphs, compact rows and auto-restart over a pool twice the slot count against the eager single group."""
    import torch
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    W, H, bin_h, N, sims, games, n_inst = 10, 10, 5, 8, 10, 4, 8
    game, args = rollout_game(W, H, N, sims)
    wh = br.instances(W, bin_h, N, n_inst)
    area = np.full(n_inst, W * bin_h, np.int32)
    runs = []
    for groups, graph, compact in ((2, True, True), (1, False, False)):
        sp = BatchedSelfPlay(game, None, args, games=games, move_rule=_lib.MOVE_INCUMBENT, seed=br.SEED, groups=groups, use_graph=graph, compact_rows=compact,
                             tie_salt=br.SALT, record_packings=True, record_best=True, playout_incumbents=True, evaluator="rollout", playouts=PLAYOUTS)
        ids, outcome, score, moves, _ = sp.run(wh, area, br.BUF)
        followed = sp.counters()["followed_moves"]
        packs, best = sp.pop_packings(), sp.pop_best_packings()
        for p, played in zip(best, packs):
            p.played = played
        check_followed_packings(best, n_inst)
        runs.append(dict(result=(ids, outcome, score, moves), packs=packs, best=best, followed=followed))
        sp.close()
    a, b = runs
    assert a["followed"] == b["followed"] > 0
    for x, y in zip(a["result"], b["result"]):
        assert np.array_equal(x, y)
    assert a["packs"] == b["packs"]
    for p, q in zip(a["best"], b["best"]):
        assert p == q and (p.prefix, p.updates, p.tree_moves, p.playout) == (q.prefix, q.updates, q.tree_moves, q.playout)
    refs = playout_refs(1, "uniform")  # the same instances, seed, salt and buffer: the pool's episodes are the reference's
    for g, ref in enumerate(refs):
        assert a["packs"][g].actions.tolist() == ref["actions"] and a["packs"][g].score == ref["score"], g
    torch.cuda.synchronize()


def test_pack_follows_the_incumbent_with_and_without_best():
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    from resource_packing_self_play_amd.solve import pack
    W, H, bin_h, N, sims, games = 10, 10, 5, 8, 10, 8
    game, args = rollout_game(W, H, N, sims)
    wh = br.instances(W, bin_h, N, games)
    kw = dict(item_wh=wh, total_area=np.full(games, W * bin_h, np.int32), rewards_list=br.BUF, move_rule=_lib.MOVE_INCUMBENT, evaluator="rollout",
              playouts=PLAYOUTS, seed=br.SEED, tie_salt=br.SALT)
    best = pack(game, None, args, best=True, **kw)
    check_followed_packings(best, games)
    played = pack(game, None, args, **kw)  # without best: the driver still keeps the incumbents, the played packings come back
    assert played == [p.played for p in best] and all(p.prefix is None for p in played)
    sp = BatchedSelfPlay(game, None, args, games=games, move_rule=_lib.MOVE_ARGMAX_FIRST, record_packings=True, evaluator="rollout", playouts=PLAYOUTS,
                         seed=br.SEED, tie_salt=br.SALT)
    with pytest.raises(RuntimeError, match="record_best"):
        pack(game, None, args, driver=sp, **kw)
    with pytest.raises(ValueError, match="record_best"):
        sp.set_move_rule(_lib.MOVE_INCUMBENT)
    sp.set_record_best(True)
    sp.set_move_rule(_lib.MOVE_INCUMBENT)
    with pytest.raises(ValueError, match="MOVE_INCUMBENT"):
        sp.set_record_best(False)
    assert sp.record_best and sp.move_rule == _lib.MOVE_INCUMBENT
    assert pack(game, None, args, driver=sp, **kw) == played
    sp.close()
    with pytest.raises(ValueError, match="record_best"):
        BatchedSelfPlay(game, None, args, games=games, move_rule=_lib.MOVE_INCUMBENT, evaluator="rollout", playouts=PLAYOUTS)
    with pytest.raises(ValueError, match="MOVE_INCUMBENT"):
        _lib.Engine(W, H, N, 1, sims, move_rule=_lib.MOVE_INCUMBENT)


# ---- 4. N > 64: the second lane pair of the prefix comparison ---------------------------------------------------------------------------------
def test_more_than_64_items():
    """Slot 0 plays under `hashed` and follows at moves 66 to 69, slot 1 under `uniform` at 68 and 69 (the table evaluators do not
    read the episode id, so both slots are the reference's episode)."""
    refs = [dict(mi.big_episode(kind, want_tree=True)) for kind in br.KINDS]
    assert [sum(r["followed"][64:]) for r in refs] == [4, 2]
    wh = mi.big_instance()
    eng = follow_engine(mi.BIG_W, mi.BIG_H, mi.BIG_N, 2, mi.BIG_SIMS)
    eng.begin_episodes(np.stack([wh, wh]), [mi.BIG_AREA] * 2, episode_id=[0, 1])
    run_until_idle(eng, table_evaluator(mi.BIG_W, mi.BIG_N))
    check_all(eng, refs, "12x12/70")
    eng.close()


# ---- 5. the rule switched on in the middle of an episode --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,game,k", SWITCHES)
def test_mid_episode_switch(shape, game, k):
    """RP_MOVE_ARGMAX_FIRST up to move k, then rp_set_move_rule(4): in the first three the record holds an incumbent whose line does not
    pass through the root (condition 4), in the last one it does and is followed from move k on."""
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, games = br.SHAPES[shape]
    ref = mi.probe(shape, game, switch_at=k, want_tree=True)[1]
    eng = follow_engine(W, H, N, 1, sims)
    eng.set_move_rule(_lib.MOVE_ARGMAX_FIRST)
    eng.begin_episodes(br.instances(W, bin_h, N, games)[game][None], [W * bin_h], episode_id=[0])
    evaluate = table_evaluator(W, N, lambda s: br.KINDS[game % 2])
    switched = False
    for _ in range(10 ** 6):
        n = eng.search_step()
        if n:
            rows, rem, slots = eng.leaf_states(n)
            eng.commit_eval_host(*evaluate(rows, rem, slots))
        ph, _, mv, _ = eng.status()
        if not switched and mv[0] >= k:  # move k - 1 has been played, move k has not: one move per search step
            assert mv[0] == k
            eng.set_move_rule(_lib.MOVE_INCUMBENT)
            switched = True
        if n == 0 and ph[0] not in (_lib.PHASE_RUNNING, _lib.PHASE_MOVE_READY):
            break
    assert switched
    check_all(eng, [ref], "switch at %d" % k, from_start=False)
    eng.close()


# ---- 6. the device rule reads the record the host sees ----------------------------------------------------------------------------------------
def watched_run(eng, evaluate, host_rule):
    """Runs the episodes to the end; at every move of every slot -> {(slot, move): (root counts, running incumbent)}.  host_rule: the
    context is RP_MOVE_EXTERNAL and the rule is applied here, from rp_incumbents and rp_root_counts, through rp_advance_roots."""
    from resource_packing_self_play_amd import _lib
    seen, played = {}, {g: [] for g in range(eng.G)}
    for _ in range(10 ** 6):
        n = eng.search_step()
        if n:
            rows, rem, slots = eng.leaf_states(n)
            eng.commit_eval_host(*evaluate(rows, rem, slots))
        ph, _, mv, _ = eng.status()
        for g in np.flatnonzero(ph == _lib.PHASE_MOVE_READY):
            g, m = int(g), int(mv[g])
            if (g, m) in seen:
                continue
            inc = {f: v[0] for f, v in eng.incumbents(g, 1).items()}
            counts = eng.root_counts(g, 1)[0]
            seen[(g, m)] = (counts, inc)
            if host_rule:
                line = [int(a) for a in inc["action"][:max(int(inc["moves"]), 0)]]
                follow = int(inc["moves"]) > m and float(inc["score"]) > 0 and line[:m] == played[g]
                action = line[m] if follow else int(np.argmax(counts))
                played[g].append(action)
                eng.advance_roots([action], first=g)
        if n == 0 and not np.isin(eng.status()[0], (_lib.PHASE_RUNNING, _lib.PHASE_MOVE_READY, _lib.PHASE_WAIT_EVAL)).any():
            return seen


@pytest.mark.parametrize("shape", [1, 4])
def test_host_rule_through_advance_roots_is_the_device_rule(shape):
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, games = br.SHAPES[shape]
    wh, area = br.instances(W, bin_h, N, games), np.full(games, W * bin_h, np.int32)
    runs = []
    for host_rule in (False, True):
        eng = follow_engine(W, H, N, games, sims)
        if host_rule:
            eng.set_move_rule(_lib.MOVE_EXTERNAL)
        eng.begin_episodes(wh, area, episode_id=np.arange(games))
        seen = watched_run(eng, table_evaluator(W, N), host_rule)
        runs.append((seen, finished(eng), eng.counters()["followed_moves"]))
        eng.close()
    (dev_seen, dev_fin, dev_followed), (host_seen, host_fin, host_followed) = runs
    refs = table_refs(shape)
    assert dev_followed == sum(r["n_followed"] for r in refs) > 0 and host_followed == 0
    assert sorted(dev_seen) == sorted(host_seen) == sorted((g, m) for g, r in enumerate(refs) for m in range(len(r["actions"])))
    for key in dev_seen:
        (c0, i0), (c1, i1) = dev_seen[key], host_seen[key]
        assert np.array_equal(c0, c1) and np.array_equal(c0, refs[key[0]]["fallback_counts"][key[1]]), key
        for f in i0:
            assert np.array_equal(i0[f], i1[f]), (key, f)
        check_incumbent(i0, refs[key[0]]["running"][key[1]], "running %s" % (key,))
    for g in range(games):
        for f in dev_fin[g]:
            assert np.array_equal(dev_fin[g][f], host_fin[g][f]), (g, f)


# ---- 7. examples ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onehot", [True, False])
def test_examples_under_the_rule(onehot):
    """One example per move.  One-hot: hot at the played action, a followed action the search never visited included; otherwise the row is
    the root's visit counts, whatever was played."""
    W, H, bin_h, N, sims, games = br.SHAPES[1]
    refs = playout_refs(1, "uniform")
    unvisited = [(g, m) for g, r in enumerate(refs) for m, f in enumerate(r["followed"]) if f and int(r["fallback_counts"][m][r["actions"][m]]) == 0]
    assert unvisited
    eng = follow_engine(W, H, N, games, sims, playouts=True, onehot=onehot, max_examples=games * N)
    eng.begin_episodes(br.instances(W, bin_h, N, games), np.full(games, W * bin_h, np.int32), episode_id=np.arange(games))
    rollout_loop(eng)
    t = {k: v.cpu().numpy() for k, v in eng.examples_packed("cuda").items()}
    assert sorted(zip(t["episode"].tolist(), t["move"].tolist())) == [(g, m) for g, r in enumerate(refs) for m in range(len(r["actions"]))]
    for e in range(len(t["episode"])):
        g, m = int(t["episode"][e]), int(t["move"][e])
        lo, n = int(t["sp_off"][e]), int(t["sp_n"][e])
        row = np.zeros(W * N, np.uint32)
        row[t["sp_act"][lo:lo + n].astype(np.uint16)] = t["sp_cnt"][lo:lo + n].astype(np.uint32)
        if onehot:
            assert n == 1 and int(t["sp_act"][lo]) == refs[g]["actions"][m] and int(t["sp_cnt"][lo]) == 1, (g, m)
        else:
            assert np.array_equal(row, refs[g]["fallback_counts"][m]), (g, m)
        assert int(t["value"][e]) == refs[g]["outcome"]
    eng.close()


# ---- 8. the contract of the calls -------------------------------------------------------------------------------------------------------------
def test_contract_of_the_calls():
    from resource_packing_self_play_amd import _lib
    W, H, bin_h, N, sims, games = br.SHAPES[1]
    wh, area = br.instances(W, bin_h, N, games), np.full(games, W * bin_h, np.int32)
    L = _lib.load()
    assert L.rp_version() == 10 == _lib.ABI_VERSION and _lib.MOVE_INCUMBENT == 4
    # rp_create with the rule: a new context keeps no incumbents yet
    cfg = _lib.RpConfig(_lib.ABI_VERSION, W, H, N, games, sims, 1.0, br.ALPHA, 0, 0, _lib.MOVE_INCUMBENT, 0, 0, 0, br.SEED, br.SALT, 0, 0, None, 0, 0)
    h = C.c_void_p()
    assert L.rp_create(C.byref(cfg), C.byref(h)) == _lib.ERR_ARG and not h.value and b"RP_MOVE_INCUMBENT" in L.rp_last_error(None)

    def episodes(eng, policy):
        """Plays the instances; -> (finished records, followed moves since the last call); checks them against the existing references
        when `policy` names one."""
        eng.begin_episodes(wh, area, episode_id=np.arange(games))
        run_until_idle(eng, table_evaluator(W, N))
        got = finished(eng) if eng.incumbent else None
        if policy is not None:
            for g in range(games):
                played, outcome, score, ref = br.oracle_episode(W, H, N, wh[g], W * bin_h, br.BUF, br.KINDS[g % 2], sims, policy, br.SEED, g)
                assert (got[g]["p_action"], got[g]["p_outcome"], got[g]["p_score"]) == (played, outcome, score), g
                assert (float(got[g]["score"]), int(got[g]["updates"])) == (ref["score"], ref["updates"]) and np.array_equal(got[g]["board"], ref["rows"])
        return got, eng.counters(reset=True)["followed_moves"]

    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=br.ALPHA, move_rule=_lib.MOVE_SAMPLE, seed=br.SEED, tie_salt=br.SALT)
    eng.set_rank_buffer(br.BUF)
    eng.set_trace(True)
    # the rule while incumbents are off: refused, rule and incumbents as they were
    with pytest.raises(_lib.EngineError) as ei:
        eng.set_move_rule(_lib.MOVE_INCUMBENT)
    assert ei.value.code == _lib.ERR_STATE and "incumbent" in str(ei.value) and eng.move_rule == _lib.MOVE_SAMPLE
    with pytest.raises(_lib.EngineError) as ei:
        eng.incumbents()
    assert ei.value.code == _lib.ERR_ARG
    eng.set_incumbent(True)
    assert episodes(eng, br.SAMPLE)[1] == 0  # still RP_MOVE_SAMPLE
    # a rule that does not exist: refused as before, the rule stays
    eng.set_move_rule(_lib.MOVE_INCUMBENT)
    with pytest.raises(_lib.EngineError) as ei:
        eng.set_move_rule(5)
    assert ei.value.code == _lib.ERR_ARG and eng.move_rule == _lib.MOVE_INCUMBENT
    # the incumbents switched off under the rule: refused, both stay
    with pytest.raises(_lib.EngineError) as ei:
        eng.set_incumbent(False)
    assert ei.value.code == _lib.ERR_STATE and "RP_MOVE_INCUMBENT" in str(ei.value) and eng.incumbent
    # outside moves under the rule: refused
    eng.begin_episodes(wh, area, episode_id=np.arange(games))
    with pytest.raises(_lib.EngineError) as ei:
        eng.advance_roots([0] * games)
    assert ei.value.code == _lib.ERR_STATE and eng.status()[2].tolist() == [0] * games
    got, followed = episodes(eng, None)  # the rule is in force, the incumbents are on
    refs = table_refs(1)
    assert followed == sum(r["n_followed"] for r in refs) > 0
    for g, ref in enumerate(refs):
        check_episode(got[g], ref, "game %d" % g)
    # back to the rules that read the counts alone: the existing references, and the counter does not move
    for rule, policy in ((_lib.MOVE_ARGMAX_FIRST, br.ARGMAX_FIRST), (_lib.MOVE_SAMPLE, br.SAMPLE)):
        eng.set_move_rule(rule)
        assert episodes(eng, policy)[1] == 0
    eng.set_move_rule(_lib.MOVE_ARGMAX_DRAW)  # the oracle has no policy for the drawn argmax (best_ref: ARGMAX_FIRST and SAMPLE only), so
    assert episodes(eng, None)[1] == 0  # there is no reference episode to compare with: the counter alone is checked
    eng.set_incumbent(False)  # allowed again
    eng.close()
    # ... and with playouts as candidates: best_playout_ref's episode
    eng = follow_engine(W, H, N, 2, sims, playouts=True)
    eng.set_move_rule(_lib.MOVE_SAMPLE)
    eng.begin_episodes(wh[:2], area[:2], episode_id=np.arange(2))
    rollout_loop(eng)
    got = finished(eng)
    for g in range(2):
        ref = bp.probe(1, g)[1]
        assert (got[g]["p_action"], got[g]["p_score"]) == (ref["played"]["actions"].tolist(), ref["played"]["score"]), g
        assert (float(got[g]["score"]), int(got[g]["updates"]), int(got[g]["playout"])) == (ref["score"], ref["updates"], ref["playout"]), g
    assert eng.counters()["followed_moves"] == 0
    eng.close()
