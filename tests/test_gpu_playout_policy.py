"""GPU parity of the playout policy (rp_set_playout_policy / rp_playout_policy, BatchedSelfPlay's / solve.pack's / solve.random_scores'
playout_policy) against the Python restatement of its rule over the CPU oracle (tests/playout_policy_ref.py).  Everything is compared bit
for bit; tests/test_playout_policy_cpu.py proves that the states used here reach every branch of the weighted pick."""
import functools

import numpy as np
import pytest

import best_playout_ref as bp
import best_ref as br
import evaluators as ev
import initial_ref as ir
import oracle_lib as orc
import playout_policy_ref as pp
import rollout_ref as rr
from engine_util import assert_trees_equal, tree_as_dict

pytestmark = pytest.mark.gpu
SEED, SALT = pp.GPU_SEED, pp.GPU_SALT


def engine(name, games=1, sims=1, **kw):
    from resource_packing_self_play_amd import _lib
    W, H, N, _ = rr.GEOMETRIES[name]
    return _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=rr.ALPHA, seed=SEED, tie_salt=SALT, **kw)


def state_arrays(states):
    rows = np.stack([ev.pack_board(s[2]) for s in states]); rem = np.stack([s[3] for s in states])
    wh = np.stack([s[0] for s in states]); area = np.array([s[1] for s in states], np.int32)
    return rows, rem, wh, area, wh[:, :, 1].max(axis=1).astype(np.int32), np.array([s[4] for s in states], np.uint64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's playouts of pp.gpu_states(name), computed once -> (states, {(policy, state, playout): (moves, final board cells,
    final rem, action list)})."""
    W, H, N, _ = rr.GEOMETRIES[name]
    states, out = pp.gpu_states(name), {}
    for policy in pp.GPU_POLICIES:
        for b, s in enumerate(states):
            for j in range(pp.GPU_PLAYOUTS):
                trace = []
                m, fb, fr = pp.playout_path(W, H, N, s[2], s[3], s[0], SEED, s[4], j, trace=trace, policy=policy)
                out[(policy, b, j)] = (m, fb, fr, [t[3] for t in trace])
    return states, out


# ---- 1. the stateless batch and the action lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rr.GEOMETRIES))
def test_rollout_states_and_paths_match_the_restatement(name):
    """The start, a mid-game state and a near-terminal state, 4 playouts each, under (1,1), (2,0) and (0,2), non-zero episode ids:
    outcomes, scores (float64 equality), move counts, final boards and action lists; the three buffers on the smallest geometry."""
    W, H, N, _ = rr.GEOMETRIES[name]
    states, want = reference(name)
    B, K = len(states), pp.GPU_PLAYOUTS
    rows, rem, wh, area, max_h, ids = state_arrays(states)
    assert B == 3 and ids.all()
    eng = engine(name)
    for policy in pp.GPU_POLICIES:
        eng.set_playout_policy(*policy)
        assert eng.playout_policy() == policy
        action, moves_p = eng.rollout_paths(rows, rem, wh, K, episode_id=ids)
        for label, buf in pp.gpu_buffers(name).items():
            outcome, score, moves, board = eng.rollout_states(rows, rem, wh, area, max_h, buf, rr.ALPHA, K, episode_id=ids)
            for b in range(B):
                for j in range(K):
                    m, fb, fr, acts = want[(policy, b, j)]
                    e, r = rr.rank(W, H, fb, fr, int(area[b]), int(max_h[b]), buf, SALT)
                    where = "%s, policy %s, buffer %s, state %d, playout %d" % (name, policy, label, b, j)
                    assert moves[b, j] == m == moves_p[b, j], where
                    assert np.array_equal(board[b, j], ev.pack_board(fb)), where
                    assert score[b, j] == r and outcome[b, j] == e, where
                    assert [int(a) for a in action[b, j, :m]] == acts and not action[b, j, m:].any(), where
    eng.close()


# ---- 2. a whole search under (2, 0) ----------------------------------------------------------------------------------------------------------
POLICY_SEARCH = (2, 0)
SEARCH_SIMS, SEARCH_K = 24, 3
SEARCH_CASES = {"10x10/8": None, "12x12/70": 3}  # geometry -> moves after whose search the comparison stops (None: the whole episode)


def _game_args(W, H, N, sims):
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=sims, cpuct=1, alpha=rr.ALPHA, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


def search_instance(name):
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area = rr.make_items(name, np.random.default_rng(SEARCH_SIMS + N))
    return wh, area, rr.BUFFERS["zeros"] if name == "12x12/70" else rr.BUFFERS["mixed"], 4100 + N


@functools.lru_cache(maxsize=None)
def oracle_search(name, sample):
    """OracleMCTS with the weighted restatement as evaluator, played move by move -> (root counts of every searched move, tree dump)."""
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = search_instance(name)
    m = pp.oracle(W, H, N, wh, area, buf, SEED, SALT, eid, SEARCH_K, POLICY_SEARCH)
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    counts = []
    while orc.has_valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem):
        c = m.action_counts(board, rem, SEARCH_SIMS)
        counts.append(c)
        if len(counts) == SEARCH_CASES[name]:
            break
        if sample:  # RP_MOVE_SAMPLE, as initial_ref.play_from draws it
            r = rr.umulhi(orc.lib().orc_sample_u64(SEED, eid, len(counts) - 1), int(c.sum(dtype=np.uint64)))
            action = int(np.searchsorted(np.cumsum(c.astype(np.uint64)), r, side="right"))
        else:
            action = int(np.argmax(c))
        rc, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, action)
        assert rc == 0
    dump = m.dump()
    m.close()
    return counts, dump


def watch(eng, counts, cut):
    """Behind a wave: the root counts of a move whose search is complete, once per move -> True when the comparison ends."""
    from resource_packing_self_play_amd import _lib
    ph, _, mv, _ = eng.status()
    if int(ph[0]) == _lib.PHASE_MOVE_READY and int(mv[0]) == len(counts):
        counts.append(eng.root_counts()[0].copy())
        return cut is not None and len(counts) == cut
    return int(ph[0]) not in (_lib.PHASE_RUNNING, _lib.PHASE_WAIT_EVAL, _lib.PHASE_MOVE_READY)


def run_eager(name, rule):
    """rp_search_step -> rp_rollout_eval -> rp_commit_eval on one engine."""
    import torch
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = search_instance(name)
    eng = engine(name, sims=SEARCH_SIMS, move_rule=rule, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_playout_policy(*POLICY_SEARCH)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh[None], [area], episode_id=[eid])
    pi = torch.zeros((1, W * N), device="cuda"); v = torch.zeros(1, device="cuda")
    counts = []
    for _ in range(100000):
        if eng.search_step():
            eng.rollout_eval(v.data_ptr(), 1, SEARCH_K, pi_ptr=pi.data_ptr())
            eng.commit_eval(pi.data_ptr(), v.data_ptr())
        elif watch(eng, counts, SEARCH_CASES[name]):
            break
    eng.check()
    tree = tree_as_dict(eng.dump_tree(0))
    eng.close()
    return counts, tree


def run_graph(name, rule):
    """The captured wave of BatchedSelfPlay, one instance on one slot."""
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = search_instance(name)
    game, args = _game_args(W, H, N, SEARCH_SIMS)
    sp = BatchedSelfPlay(game, None, args, games=1, groups=1, move_rule=rule, seed=SEED, tie_salt=SALT, evaluator="rollout", playouts=SEARCH_K,
                         use_graph=True, reclaim=False, playout_policy=POLICY_SEARCH)  # reclaim off: the oracle keeps every node
    assert sp.eng.playout_policy() == POLICY_SEARCH
    sp.start(wh[None], np.array([area], np.int32), buf, first_id=eid)
    counts = []
    for _ in range(100000):
        sp.step()
        if watch(sp.eng, counts, SEARCH_CASES[name]):
            break
    assert sp.groups[0].graph is not None
    sp.eng.check()
    tree = tree_as_dict(sp.eng.dump_tree(0))
    sp.close()
    return counts, tree


@pytest.mark.parametrize("sample", [False, True], ids=["argmax_first", "sample"])
@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_search_under_width2_matches_the_oracle(name, sample):
    from resource_packing_self_play_amd import _lib
    rule = _lib.MOVE_SAMPLE if sample else _lib.MOVE_ARGMAX_FIRST
    want_counts, want_tree = oracle_search(name, sample)
    runs = {"eager": run_eager(name, rule), "graph": run_graph(name, rule)}
    for how, (counts, tree) in runs.items():
        assert len(counts) == len(want_counts), how
        for k, (c, w) in enumerate(zip(counts, want_counts)):
            assert np.array_equal(c, w), "%s, %s: move %d" % (name, how, k)
        assert_trees_equal(tree, want_tree, "%s, %s" % (name, how))
    assert_trees_equal(runs["eager"][1], runs["graph"][1], name + ": eager against graph")
    # the policy matters here: the uniform restatement searches another tree
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = search_instance(name)
    m = rr.oracle(W, H, N, wh, area, buf, SEED, SALT, eid, SEARCH_K)
    uniform = m.action_counts(np.zeros((H, W), np.uint8), np.ones(N, np.uint8), SEARCH_SIMS)
    m.close()
    assert not np.array_equal(uniform, want_counts[0])


# ---- 3. playout incumbents under (1, 1) ------------------------------------------------------------------------------------------------------
POLICY_INC = (1, 1)


def test_playout_incumbents_replay_under_the_policy(monkeypatch):
    """The offer's winner is played again under the policy that scored it: every finished record is best_playout_ref's with the
    weighted functions in rollout_ref's place, and its action list replays through solve.replay_rows to its board and score."""
    import test_gpu_best_playout as tb
    from resource_packing_self_play_amd import solve
    pp.under(monkeypatch, POLICY_INC)
    W, H, bin_h, N, sims, games = br.SHAPES[1]
    wh = br.instances(W, bin_h, N, games)
    area = np.full(games, W * bin_h, np.int32)
    refs = [bp.episode(W, H, N, wh[g], int(area[g]), br.BUF, sims, bp.SAMPLE, br.SEED, br.SALT, g, bp.PLAYOUTS) for g in range(games)]
    eng = tb.make_engine(W, H, N, games, sims, tb.rules(bp.SAMPLE))
    eng.set_trace(True); eng.set_incumbent(True); eng.set_incumbent_playouts(True)
    eng.set_playout_policy(*POLICY_INC)
    eng.begin_episodes(wh, area, episode_id=np.arange(games))
    tb.eager_loop(eng, bp.PLAYOUTS)
    done = tb.finished(eng)
    eng.close()
    assert sorted(done) == list(range(games))
    from_playouts = 0
    for g, ref in enumerate(refs):
        got, played = done[g], ref["played"]
        assert (got["p_action"], got["p_outcome"], got["p_score"]) == ([int(a) for a in played["actions"]], played["outcome"], played["score"]), g
        tb.check_record(got, ref, W, H, N, ref["sizes"], played["actions"], "game %d" % g)
        m, tm, j = int(got["moves"]), int(got["tree_moves"]), int(got["playout"])
        _, board = solve.replay_rows(W, H, wh[g], got["action"][:m])
        assert np.array_equal(board, got["board"]), g
        assert orc.ranked_reward(W, H, ev.unpack_board(board, W), int(area[g]), ir.default_max_h(wh[g], np.ones(N)), br.BUF, br.ALPHA)[1] == float(got["score"]), g
        assert float(got["score"]) >= got["p_score"], g
        if j >= 0:  # the restatement's playout j from the leaf reached after tree_moves actions
            _, leaf = solve.replay_rows(W, H, wh[g], got["action"][:tm])
            leaf_rem = np.ones(N, np.uint8); leaf_rem[[int(a) // W for a in got["action"][:tm]]] = 0
            trace = []
            mv, fb, _ = pp.playout_path(W, H, N, ev.unpack_board(leaf, W), leaf_rem, wh[g], br.SEED, g, j, trace=trace, policy=POLICY_INC)
            assert [t[3] for t in trace] == [int(a) for a in got["action"][tm:m]] and mv == m - tm, g
            assert np.array_equal(ev.pack_board(fb), got["board"]), g
            from_playouts += 1
    assert from_playouts >= 1, "no incumbent came from a playout"


# ---- 4. back to uniform -----------------------------------------------------------------------------------------------------------------------
def test_uniform_after_a_weighted_policy_is_the_untouched_context():
    """(1, 1) and then (0, 0): rollout_states, rollout_paths and a short search equal those of a context that never called the setter."""
    import torch
    from resource_packing_self_play_amd import _lib
    name, sims, K = "10x10/8", 16, 3
    W, H, N, _ = rr.GEOMETRIES[name]
    states, _ = reference(name)
    rows, rem, wh, area, max_h, ids = state_arrays(states)
    runs = []
    for touch in (False, True):
        eng = engine(name, sims=sims, move_rule=_lib.MOVE_SAMPLE, stream=torch.cuda.current_stream().cuda_stream)
        weighted = None
        if touch:
            eng.set_playout_policy(1, 1)
            weighted = eng.rollout_states(rows, rem, wh, area, max_h, rr.BUFFERS["mixed"], rr.ALPHA, K, episode_id=ids)
            eng.set_playout_policy(0, 0)
        assert eng.playout_policy() == (0, 0)
        out = list(eng.rollout_states(rows, rem, wh, area, max_h, rr.BUFFERS["mixed"], rr.ALPHA, K, episode_id=ids))
        out += list(eng.rollout_paths(rows, rem, wh, K, episode_id=ids))
        if weighted is not None:
            assert not np.array_equal(weighted[3], out[3]), "the weighted playouts ended on the uniform ones' boards"
        eng.set_rank_buffer(rr.BUFFERS["mixed"])
        eng.begin_episodes(wh[:1], area[:1], episode_id=[77])
        pi = torch.zeros((1, W * N), device="cuda"); v = torch.zeros(1, device="cuda")
        for _ in range(100000):
            if eng.search_step():
                eng.rollout_eval(v.data_ptr(), 1, K, pi_ptr=pi.data_ptr())
                eng.commit_eval(pi.data_ptr(), v.data_ptr())
            elif int(eng.status()[0][0]) not in (_lib.PHASE_RUNNING, _lib.PHASE_MOVE_READY):
                break
        eng.check()
        out += [np.asarray(x) for x in eng.pop_finished()]
        runs.append((out, tree_as_dict(eng.dump_tree(0))))
        eng.close()
    assert len(runs[0][0]) == len(runs[1][0])
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert_trees_equal(runs[0][1], runs[1][1], "touched against untouched")
    s = states[0]  # and both are rollout_ref's uniform playouts
    assert runs[0][0][1][0, 0] == rr.playout(W, H, N, s[2], s[3], s[0], s[1], rr.BUFFERS["mixed"], SEED, SALT, s[4], 0)[1]


# ---- 5. refusals, the getter, the public API ---------------------------------------------------------------------------------------------------
def test_setter_refusals_and_getter():
    from resource_packing_self_play_amd import _lib
    name = "10x10/8"
    wh, area = rr.make_items(name, np.random.default_rng(1))
    eng = engine(name, move_rule=_lib.MOVE_ARGMAX_FIRST)
    assert eng.playout_policy() == (0, 0)  # the default
    for pair in pp.NAMES.values():
        eng.set_playout_policy(*pair)
        assert eng.playout_policy() == pair
    for bad in ((3, 0), (2, 1), (-1, 0), (0, 3), (0, -1), (1, 2)):
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_playout_policy(*bad)
        assert ei.value.code == _lib.ERR_ARG
        assert eng.playout_policy() == (0, 2)  # a refused call changes nothing
    eng.begin_episodes(wh[None], [area])
    assert eng.search_step() == 1  # the slot waits for its root's evaluation
    for pair in ((1, 1), (0, 0), (0, 2)):
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_playout_policy(*pair)
        assert ei.value.code == _lib.ERR_STATE and "middle of an episode" in str(ei.value)
    assert eng.playout_policy() == (0, 2)
    eng.close()


def test_python_api_names_and_refusals():
    from resource_packing_self_play_amd import solve
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    from test_gpu_packings import cnn_setup
    name = "10x10/8"
    W, H, N, _ = rr.GEOMETRIES[name]
    game, args = _game_args(W, H, N, 8)
    rng = np.random.default_rng(6)
    wh = np.stack([rr.make_items(name, rng)[0] for _ in range(3)])
    board0, rem0 = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    for bad in ("depth", (3, 0), (2, 1), (-1, 0), 1):
        with pytest.raises(ValueError):
            solve.random_scores(game, item_wh=wh, playouts=2, playout_policy=bad)
        with pytest.raises(ValueError):
            solve.pack(game, None, args, item_wh=wh, evaluator="rollout", playouts=2, playout_policy=bad)
        with pytest.raises(ValueError):
            BatchedSelfPlay(game, None, args, games=2, evaluator="rollout", playout_policy=bad)
    cnn_game, nnet, cnn_args = cnn_setup(W, H, N, 8)
    for kw in (dict(playout_policy="width2"), dict(playout_policy=(1, 1), evaluator="cnn")):  # the CNN runs no playouts
        with pytest.raises(ValueError):
            solve.pack(cnn_game, nnet, cnn_args, item_wh=wh, **kw)
        with pytest.raises(ValueError):
            BatchedSelfPlay(cnn_game, nnet, cnn_args, games=2, **kw)
    # a name is its pair, and the scores are the restatement's
    scores = solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED, playout_policy="width2")
    assert np.array_equal(scores, solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED, playout_policy=(2, 0)))
    want = [[pp.playout(W, H, N, board0, rem0, wh[i], int(wh[i, :, 0].astype(int) @ wh[i, :, 1]), [], SEED, SALT, i, j, policy=(2, 0))[1] for j in range(3)]
            for i in range(3)]
    assert np.array_equal(scores, np.array(want))
    assert np.array_equal(solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED, playout_policy="uniform"),
                          solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED))
    # pack under a policy plays the oracle's episodes with the weighted evaluator
    buf = scores.reshape(-1)
    packs = solve.pack(game, None, args, item_wh=wh, evaluator="rollout", playouts=3, rewards_list=buf, seed=SEED, tie_salt=SALT, playout_policy="area",
                       best=True, playout_incumbents=True)
    for i, p in enumerate(packs):
        m = pp.oracle(W, H, N, wh[i], W * H, buf, SEED, SALT, i, 3, (1, 1))
        actions, _, o, s = m.play_episode(8, policy=0, want_counts=False)
        m.close()
        assert list(p.played.actions) == [int(x) for x in actions] and (p.played.outcome, p.played.score) == (o, s), i
        assert p.score >= p.played.score
        p.layout()
