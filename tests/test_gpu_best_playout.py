"""GPU parity of the playout incumbents (rp_set_incumbent_playouts / rp_pop_finished_best_playouts / rp_incumbent_sources /
rp_rollout_paths, BatchedSelfPlay's playout_incumbents, solve.pack's playout_incumbents=True) against the incumbent computed from the CPU
oracle with every playout as a candidate (tests/best_playout_ref.py).  Every comparison is exact: integers, and doubles produced by the
same arithmetic."""
import functools

import numpy as np
import pytest

import best_playout_ref as bp
import best_ref as br
import evaluators as ev
import oracle_lib as orc
import rollout_ref as rr

pytestmark = pytest.mark.gpu
ROLLOUT_SEED, ROLLOUT_SALT = 20251, 77  # of the rollout_ref.GEOMETRIES cases, as tests/test_gpu_rollout.py plays them


def make_engine(W, H, N, games, sims, rule, seed=br.SEED, salt=br.SALT, buf=br.BUF, **kw):
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=br.ALPHA, move_rule=rule, seed=seed, tie_salt=salt,
                      stream=torch.cuda.current_stream().cuda_stream, **kw)
    eng.set_rank_buffer(buf)
    return eng


def rules(policy):
    from resource_packing_self_play_amd import _lib
    return {bp.SAMPLE: _lib.MOVE_SAMPLE, bp.ARGMAX_FIRST: _lib.MOVE_ARGMAX_FIRST}[policy]


def eager_loop(eng, playouts, watch_move=None, stop_at_watch=False, evals=1):
    """rp_search_step -> rp_rollout_eval (`evals` times) -> rp_commit_eval until every slot is done.  watch_move: the running incumbent
    of every slot is read once, when the search of that move (from 0) is complete -> {episode id: record}."""
    import torch
    from resource_packing_self_play_amd import _lib
    G, A = eng.G, eng.A
    pi = torch.zeros((G, A), device="cuda"); v = torch.zeros(G, device="cuda")
    seen = {}
    for _ in range(10 ** 6):
        n = eng.search_step()
        if n:
            for _ in range(evals):
                eng.rollout_eval(v.data_ptr(), G, playouts, pi_ptr=pi.data_ptr())
            eng.commit_eval(pi.data_ptr(), v.data_ptr())
        ph, _, mv, ep = eng.status()
        if watch_move is not None:
            for g in np.flatnonzero((ph == _lib.PHASE_MOVE_READY) & (mv == watch_move)):
                if int(ep[g]) not in seen:
                    inc = eng.incumbents(int(g), 1); src = eng.incumbent_sources(int(g), 1)
                    seen[int(ep[g])] = {**{f: inc[f][0] for f in inc}, **{f: src[f][0] for f in src}}
            if stop_at_watch and len(seen) == G:
                break
        if n == 0 and not np.isin(ph, (_lib.PHASE_RUNNING, _lib.PHASE_MOVE_READY, _lib.PHASE_WAIT_EVAL)).any():
            break
    eng.check()
    return seen


def finished(eng):
    """-> {episode id: dict(p_outcome, p_score, p_action, best fields ...)}"""
    rec = eng.pop_finished(packings=True, best=True)
    ids, oc, sc, mv, act, best = rec[0], rec[1], rec[2], rec[3], rec[4], rec[-1]
    assert len(set(ids.tolist())) == len(ids), "an episode was recorded twice"
    return {int(i): dict(p_outcome=int(oc[k]), p_score=float(sc[k]), p_action=[int(a) for a in act[k, :int(mv[k])]], **{f: best[f][k] for f in best})
            for k, i in enumerate(ids)}


def replay(W, H, N, sizes, actions, board=None, rem=None):
    board = np.zeros((H, W), np.uint8) if board is None else np.array(board, np.uint8)
    rem = np.ones(N, np.uint8) if rem is None else np.array(rem, np.uint8)
    for a in actions:
        assert rem[int(a) // W], "action %d places an item that is gone" % a
        rc, board, rem = orc.next_state(W, H, N, board, sizes[:, 0], sizes[:, 1], rem, int(a))
        assert rc == 0
    return ev.pack_board(board), rem


def check_record(got, want, W, H, N, sizes, played, where, board=None, rem=None):
    """One record (finished or running) against a record of best_playout_ref: every field, and the three parts of the action list."""
    m, tm, prefix = int(got["moves"]), int(got["tree_moves"]), int(got["prefix"])
    assert float(got["score"]) == want["score"], (where, float(got["score"]), want["score"])
    assert (int(got["outcome"]), m, prefix, int(got["updates"]), tm, int(got["playout"])) == \
        (want["outcome"], want["moves"], want["prefix"], want["updates"], want["tree_moves"], want["playout"]), where
    assert np.array_equal(got["board"], want["rows"]), where
    action = [int(a) for a in got["action"]]
    assert not any(action[m:]) and 0 <= prefix <= tm <= m, where  # zero past the incumbent's moves
    if played is not None:
        assert action[:prefix] == [int(a) for a in played][:prefix] and prefix <= len(played), where
    at_leaf = replay(W, H, N, sizes, action[:tm], board, rem)
    if want["playout"] >= 0:
        assert action[tm:m] == want["actions"], where  # the playout's own list, exactly
        assert np.array_equal(at_leaf[0], want["leaf"][0]) and np.array_equal(at_leaf[1], want["leaf"][1]), where  # the head leads to the leaf
        final = replay(W, H, N, sizes, action[tm:m], ev.unpack_board(at_leaf[0], W), at_leaf[1])
    else:
        assert tm == m, where
        final = at_leaf
    assert np.array_equal(final[0], want["rows"]) and np.array_equal(final[1], want["rem"]), where


# ---- the cases of the search parity: computed once, shared ----------------------------------------------------------------------------------
# name -> index into best_ref.SHAPES (the probe's settings; 20x20/32 with 2 games), or a geometry of rollout_ref.GEOMETRIES (one game)
CASES = {"10x10/8 s30": 0, "10x10/8 s10": 1, "15x15/10": 2, "20x20/32": 3, "6x8/5": 4, "40x6/12": "40x6/12", "12x12/70": "12x12/70"}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(W, H, N, sims, K, policy, seed, salt, buf, wh [G, N, 2], area [G], max_moves, refs [G])"""
    key = CASES[name]
    if isinstance(key, int):
        W, H, bin_h, N, sims, games = br.SHAPES[key]
        games = 2 if name == "20x20/32" else games
        wh = br.instances(W, bin_h, N, br.SHAPES[key][5])[:games]
        c = dict(W=W, H=H, N=N, sims=sims, K=bp.PLAYOUTS, policy=bp.SAMPLE, seed=br.SEED, salt=br.SALT, buf=br.BUF, wh=wh,
                 area=np.full(games, W * bin_h, np.int32), max_moves=None)
    else:  # 64-bit rows; N > 64 cut to 3 moves, as tests/test_gpu_rollout.py plays them
        W, H, N, _ = rr.GEOMETRIES[key]
        sims, max_moves = (16, None) if key == "40x6/12" else (8, 3)
        wh, area = rr.make_items(key, np.random.default_rng(sims + N))
        c = dict(W=W, H=H, N=N, sims=sims, K=2, policy=bp.ARGMAX_FIRST, seed=ROLLOUT_SEED, salt=ROLLOUT_SALT,
                 buf=rr.BUFFERS["zeros"] if key == "12x12/70" else rr.BUFFERS["mixed"], wh=wh[None], area=np.array([area], np.int32), max_moves=max_moves)
    c["refs"] = [bp.episode(c["W"], c["H"], c["N"], c["wh"][g], int(c["area"][g]), c["buf"], c["sims"], c["policy"], c["seed"], c["salt"], g, c["K"],
                            max_moves=c["max_moves"]) for g in range(len(c["wh"]))]
    return c


def case_engine(c, playouts_on=True, **kw):
    eng = make_engine(c["W"], c["H"], c["N"], len(c["wh"]), c["sims"], rules(c["policy"]), c["seed"], c["salt"], c["buf"], **kw)
    eng.set_trace(True)
    eng.set_incumbent(True)
    if playouts_on:
        eng.set_incumbent_playouts(True)
    eng.begin_episodes(c["wh"], c["area"], episode_id=np.arange(len(c["wh"])))
    return eng


# ---- 1. the action lists of the playouts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rr.GEOMETRIES))
def test_rollout_paths_match_the_restatement(name):
    from resource_packing_self_play_amd import _lib
    from test_gpu_rollout import random_state
    W, H, N, _ = rr.GEOMETRIES[name]
    rng = np.random.default_rng(N * 19 + H)
    K = 3
    states = []  # (item sizes, area, board, rem, episode id)
    for k, depth in enumerate((0, 5) if N == 128 else (0, 2, 5, 10 ** 6)):  # 10^6 moves: played to the end -> no move left
        wh, area = rr.make_items(name, rng)
        board, rem = random_state(rng, W, H, N, wh, depth)
        states.append((wh, area, board, rem, 0 if k == 0 else 1000 * k + 7))
    eng = make_engine(W, H, N, 1, 1, 0, ROLLOUT_SEED, ROLLOUT_SALT, [])
    rows = np.stack([ev.pack_board(s[2]) for s in states]); rem = np.stack([s[3] for s in states])
    wh = np.stack([s[0] for s in states]); ids = np.array([s[4] for s in states], np.uint64)
    action, moves = eng.rollout_paths(rows, rem, wh, K, episode_id=ids)
    assert action.shape == (len(states), K, N) and action.dtype == np.uint16 and moves.shape == (len(states), K)
    area = np.array([s[1] for s in states], np.int32)
    _, _, moves_s, board_s = eng.rollout_states(rows, rem, wh, area, wh[:, :, 1].max(axis=1).astype(np.int32), [], rr.ALPHA, K, episode_id=ids)
    for b, s in enumerate(states):
        for j in range(K):
            trace = []
            m, fb, fr = rr.playout_path(W, H, N, s[2], s[3], s[0], ROLLOUT_SEED, s[4], j, trace=trace)
            where = "%s, state %d, playout %d" % (name, b, j)
            assert moves[b, j] == m == moves_s[b, j], where
            assert [int(a) for a in action[b, j, :m]] == [t[3] for t in trace] and not action[b, j, m:].any(), where
            final, _ = replay(W, H, N, s[0], action[b, j, :m], s[2], s[3])  # the list replays to the board rp_rollout_states returns
            assert np.array_equal(final, board_s[b, j]) and np.array_equal(final, ev.pack_board(fb)), where
    if N != 128:
        assert not moves[-1].any()  # the state without a legal move
    for K_bad in (0, 257):
        with pytest.raises(_lib.EngineError) as ei:
            eng.rollout_paths(rows, rem, wh, K_bad)
        assert ei.value.code == _lib.ERR_ARG
    eng.close()


# ---- 2. search parity, eager loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_playout_incumbent_matches_the_oracle(name):
    c = case(name)
    W, H, N, refs = c["W"], c["H"], c["N"], c["refs"]
    eng = case_engine(c)
    cut = c["max_moves"]
    watch = 1 if cut is None else cut - 1
    seen = eager_loop(eng, c["K"], watch_move=watch, stop_at_watch=cut is not None)
    checked = 0
    for g, got in seen.items():  # running incumbents, mid-episode: behind the search of move `watch`
        want = bp.running(refs[g], watch)
        if want is None:
            assert int(got["moves"]) == -1 and int(got["playout"]) == -1 and int(got["tree_moves"]) == 0
        else:
            played = None if refs[g]["played"] is None else refs[g]["played"]["actions"]
            check_record(got, want, W, H, N, refs[g]["sizes"], played, "%s: game %d behind move %d" % (name, g, watch))
            checked += 1
    assert checked >= 1, "no running incumbent was compared"
    if cut is None:
        done = finished(eng)
        assert sorted(done) == list(range(len(refs)))
        for g, ref in enumerate(refs):
            got, played = done[g], ref["played"]
            assert (got["p_action"], got["p_outcome"], got["p_score"]) == ([int(a) for a in played["actions"]], played["outcome"], played["score"]), g
            check_record(got, ref, W, H, N, ref["sizes"], played["actions"], "%s: game %d" % (name, g))
            assert float(got["score"]) >= ref["tree"]["score"] >= got["p_score"]
    eng.close()


# ---- 3. a tree terminal replaces a playout incumbent: the late-game starts ------------------------------------------------------------------------
def test_late_starts_end_on_the_tree_terminal():
    from resource_packing_self_play_amd import _lib
    W, H, N = bp.LATE_W, bp.LATE_H, bp.LATE_N
    inst = bp.late_instances()
    wh, boards, rem, areas = inst
    n = bp.LATE_COUNT
    # one more instance whose start is terminal: a full bin
    wh = np.concatenate([wh, wh[:1]]); boards = np.concatenate([boards, np.ones((1, H, W), np.uint8)]); rem = np.concatenate([rem, rem[:1]])
    areas = np.concatenate([areas, [W * H]]).astype(np.int32)
    rows = np.stack([ev.pack_board(b) for b in boards])
    eng = make_engine(W, H, N, 4, bp.LATE_SIMS, _lib.MOVE_ARGMAX_FIRST, auto_restart=1)
    eng.set_trace(True); eng.set_incumbent(True); eng.set_incumbent_playouts(True)
    eng.set_instance_pool(wh, areas, 0)
    eng.set_instance_initial(rows, rem)
    eng.begin_pool()
    eager_loop(eng, bp.LATE_PLAYOUTS)
    done = finished(eng)
    assert sorted(done) == list(range(n + 1))
    p_then_t = 0
    for k in range(n):
        ref, got = bp.late_episode(k, inst), done[k]
        check_record(got, ref, W, H, N, ref["sizes"], ref["played"]["actions"], "late start %d" % k, boards[k], rem[k])
        if k in bp.LATE_P_THEN_T:  # the playout came first, the tree terminal replaced it
            assert ref["sources"] == [0, -1]
            assert int(got["playout"]) == -1 and int(got["tree_moves"]) == int(got["moves"]) == 1 and int(got["updates"]) == 2
            p_then_t += 1
    assert p_then_t >= 1
    got = done[n]  # the terminal start: the incumbent is the initial state itself
    assert (int(got["moves"]), int(got["tree_moves"]), int(got["playout"]), int(got["prefix"]), int(got["updates"])) == (0, 0, -1, 0, 1)
    assert np.array_equal(got["board"], rows[n]) and not got["action"].any() and got["p_action"] == []
    eng.close()


# ---- 4. schedule independence ---------------------------------------------------------------------------------------------------------------
def _game_args(c):
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return (BinPackingGame(c["W"], c["H"], c["N"], 1),
            dotdict(numMCTSSims=c["sims"], cpuct=1, alpha=br.ALPHA, cuda=True, num_items=c["N"], num_bins=1, epochs=1, batch_size=8))


def test_graph_compact_rows_step_cap_and_groups_change_nothing():
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    c = case("10x10/8 s10")
    game, args = _game_args(c)
    sp = BatchedSelfPlay(game, None, args, games=5, move_rule=rules(c["policy"]), seed=c["seed"], tie_salt=c["salt"], evaluator="rollout", playouts=c["K"],
                         use_graph=True, compact_rows=True, step_cap=1, groups=2, record_packings=True, record_best=True, playout_incumbents=True)
    sp.run(c["wh"], c["area"], c["buf"], first_id=0)
    best, packs = sp.pop_best_packings(), sp.pop_packings()
    sp.close()
    assert [p.episode_id for p in best] == list(range(len(c["refs"])))
    for p, played, ref in zip(best, packs, c["refs"]):
        got = dict(score=p.score, outcome=p.outcome, moves=p.moves, prefix=p.prefix, updates=p.updates, board=p.board, tree_moves=p.tree_moves,
                   playout=p.playout, action=np.concatenate([p.actions, np.zeros(c["N"] - p.moves, np.int32)]))
        check_record(got, ref, c["W"], c["H"], c["N"], ref["sizes"], played.actions, "episode %d" % p.episode_id)
        assert played.actions.tolist() == [int(a) for a in ref["played"]["actions"]]
        assert played.tree_moves is None and played.playout is None
        p.layout()


def test_a_second_rollout_eval_changes_nothing():
    c = case("10x10/8 s10")
    runs = []
    for evals in (1, 2):
        eng = case_engine(c)
        eager_loop(eng, c["K"], evals=evals)
        runs.append(finished(eng))
        eng.close()
    assert sorted(runs[0]) == sorted(runs[1]) == list(range(len(c["refs"])))
    for g, rec in runs[0].items():
        for f, val in rec.items():
            assert np.array_equal(val, runs[1][g][f]), (g, f)


# ---- 5. mode off ----------------------------------------------------------------------------------------------------------------------------
def test_mode_off_is_the_tree_only_incumbent_and_costs_nothing():
    from resource_packing_self_play_amd import _lib
    c = case("10x10/8 s10")
    W, H, N, games = c["W"], c["H"], c["N"], len(c["wh"])
    eng = make_engine(W, H, N, games, c["sims"], rules(c["policy"]), c["seed"], c["salt"], c["buf"])
    eng.set_trace(True)
    traced = eng.device_bytes
    eng.set_incumbent(True)
    stride, fin_cap = (24 + 8 * H + 4 * N + 7) // 8 * 8, max(4 * games, 1024)
    assert eng.device_bytes - traced == (games + fin_cap) * stride + 16 * games  # set_incumbent alone: what it cost before
    eng.begin_episodes(c["wh"], c["area"], episode_id=np.arange(games))
    eager_loop(eng, c["K"])
    done = finished(eng)
    for g, ref in enumerate(c["refs"]):  # today's records: tree terminals only, no source fields
        got, tree = done[g], ref["tree"]
        assert "playout" not in got and "tree_moves" not in got
        assert (float(got["score"]), int(got["outcome"]), int(got["updates"])) == (tree["score"], tree["outcome"], tree["updates"]), g
        assert np.array_equal(got["board"], tree["rows"])
        br.check_actions(tree, W, H, N, c["wh"][g], got["action"][:int(got["moves"])], int(got["prefix"]), got["p_action"], where="game %d" % g)
    before = eng.device_bytes
    eng.set_incumbent_playouts(True)
    assert eng.device_bytes - before == 8 * (games + fin_cap)  # the side array, on the first enable
    eng.set_incumbent_playouts(False); eng.set_incumbent_playouts(True)
    assert eng.device_bytes - before == 8 * (games + fin_cap)  # allocated once
    eng.set_incumbent(False)  # turns the mode off too
    assert not eng.incumbent_playouts
    eng.set_incumbent(True)
    with pytest.raises(_lib.EngineError) as ei:
        eng.incumbent_sources()
    assert ei.value.code == _lib.ERR_ARG
    eng.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    from test_gpu_packings import cnn_setup
    c = case("10x10/8 s10")
    games = len(c["wh"])
    eng = make_engine(c["W"], c["H"], c["N"], games, c["sims"], rules(c["policy"]))
    with pytest.raises(_lib.EngineError) as ei:  # the mode without incumbents
        eng.set_incumbent_playouts(True)
    assert ei.value.code == _lib.ERR_STATE and "incumbent" in str(ei.value)
    eng.set_incumbent(True)
    n = C.c_int64(0)
    rc = eng.L.rp_pop_finished_best_playouts(eng.h, 1, *([None] * 16), C.byref(n))  # the pop variant while the mode is off
    assert rc == _lib.ERR_ARG and "playout incumbents are off" in eng.L.rp_last_error(eng.h).decode()
    with pytest.raises(_lib.EngineError) as ei:
        eng.incumbent_sources()
    assert ei.value.code == _lib.ERR_ARG
    eng.begin_episodes(c["wh"], c["area"], episode_id=np.arange(games))
    for on in (True, False):  # switching in mid-episode, in either direction
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_incumbent_playouts(on)
        assert ei.value.code == _lib.ERR_STATE and "middle of an episode" in str(ei.value)
    eng.close()
    game, nnet, args = cnn_setup(c["W"], c["H"], c["N"], c["sims"])
    with pytest.raises(ValueError):  # the CNN runs no playouts
        BatchedSelfPlay(game, nnet, args, games=2, record_best=True, playout_incumbents=True)
    game, args = _game_args(c)
    with pytest.raises(ValueError):  # no incumbents to feed
        BatchedSelfPlay(game, None, args, games=2, evaluator="rollout", playout_incumbents=True)


# ---- 7. the public API ----------------------------------------------------------------------------------------------------------------------
def test_pack_with_playout_incumbents():
    from resource_packing_self_play_amd.solve import pack
    c = case("10x10/8 s10")
    game, args = _game_args(c)
    kw = dict(item_wh=c["wh"], total_area=c["area"], rewards_list=c["buf"], move_rule=rules(c["policy"]), evaluator="rollout", playouts=c["K"],
              seed=c["seed"], tie_salt=c["salt"], best=True)
    on = pack(game, None, args, playout_incumbents=True, **kw)
    tree_only = pack(game, None, args, **kw)
    assert [p.episode_id for p in on] == [p.episode_id for p in tree_only] == list(range(len(c["wh"])))
    for p, q, ref in zip(on, tree_only, c["refs"]):
        p.layout(); p.played.layout(); q.layout()
        assert p.played == q.played  # what was played is unchanged
        assert p.score >= q.score >= q.played.score
        assert (p.score, p.tree_moves, p.playout) == (ref["score"], ref["tree_moves"], ref["playout"]) and q.score == ref["tree"]["score"]
        assert q.tree_moves is None and q.playout is None and p.played.tree_moves is None
    assert any(p.score > q.score for p, q in zip(on, tree_only)), "no instance improved"
    with pytest.raises(ValueError):
        pack(game, None, args, playout_incumbents=True, **dict(kw, best=False))
