"""GPU parity of the playouts' landing power (rp_set_playout_landing / rp_playout_landing, BatchedSelfPlay's / solve.pack's /
solve.random_scores' playout_landing) against the Python restatement of its rule over the CPU oracle (tests/playout_landing_ref.py).
Everything is compared bit for bit; tests/test_playout_landing_cpu.py proves that the states used here reach what they are for."""
import functools

import numpy as np
import pytest

import best_playout_ref as bp
import best_ref as br
import evaluators as ev
import initial_ref as ir
import oracle_lib as orc
import playout_landing_ref as pl
import rollout_ref as rr
from engine_util import assert_trees_equal, tree_as_dict

pytestmark = pytest.mark.gpu
SEED, SALT = pl.GPU_SEED, pl.GPU_SALT


def engine(name, games=1, sims=1, **kw):
    from resource_packing_self_play_amd import _lib
    W, H, N, _ = pl.GEOMETRIES[name]
    return _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=rr.ALPHA, seed=SEED, tie_salt=SALT, **kw)


def state_arrays(states):
    rows = np.stack([ev.pack_board(s[2]) for s in states]); rem = np.stack([s[3] for s in states])
    wh = np.stack([s[0] for s in states]); area = np.array([s[1] for s in states], np.int32)
    return rows, rem, wh, area, wh[:, :, 1].max(axis=1).astype(np.int32), np.array([s[4] for s in states], np.uint64)


# ---- 1. the stateless batch and the action lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pl.GEOMETRIES))
def test_rollout_states_and_paths_match_the_restatement(name):
    """playout_landing_ref.gpu_states under gpu_settings, 4 playouts each, non-zero episode ids: outcomes, scores (float64 equality),
    move counts, final boards and action lists."""
    W, H, N, _ = pl.GEOMETRIES[name]
    states, want = pl.gpu_states(name), pl.reference(name)
    K = pl.GPU_PLAYOUTS
    buf = rr.BUFFERS["mixed"]
    eng = engine(name)
    for b, s in enumerate(states):
        rows, rem, wh, area, max_h, ids = state_arrays([s])
        assert ids.all()
        for policy, land_pow in pl.gpu_settings(name, b):
            eng.set_playout_policy(*policy); eng.set_playout_landing(land_pow)
            assert eng.playout_policy() == policy and eng.playout_landing() == land_pow
            action, moves_p = eng.rollout_paths(rows, rem, wh, K, episode_id=ids)
            outcome, score, moves, board = eng.rollout_states(rows, rem, wh, area, max_h, buf, rr.ALPHA, K, episode_id=ids)
            for j in range(K):
                m, fb, fr, acts, _ = want[((policy, land_pow), b, j)]
                e, r = rr.rank(W, H, fb, fr, int(area[0]), int(max_h[0]), buf, SALT)
                where = "%s, policy %s, landing %d, state %d, playout %d" % (name, policy, land_pow, b, j)
                assert moves[0, j] == m == moves_p[0, j], where
                assert np.array_equal(board[0, j], ev.pack_board(fb)), where
                assert score[0, j] == r and outcome[0, j] == e, where
                assert [int(a) for a in action[0, j, :m]] == acts and not action[0, j, m:].any(), where
    eng.close()


# ---- 2. a whole search under ((2, 0), 2) ------------------------------------------------------------------------------------------------------
POLICY, LAND = pl.SEARCH_SETTING
SIMS, K_SEARCH = pl.SEARCH_SIMS, pl.SEARCH_K


def _game_args(W, H, N, sims):
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=sims, cpuct=1, alpha=rr.ALPHA, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


@functools.lru_cache(maxsize=None)
def oracle_search(name, sample, prior):
    """OracleMCTS with the restatement as evaluator, played move by move -> (root counts of every searched move, tree dump)."""
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = pl.search_instance(name)
    m = pl.oracle(W, H, N, wh, area, buf, SEED, SALT, eid, K_SEARCH, POLICY, LAND, prior)
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    counts = []
    while orc.has_valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem):
        c = m.action_counts(board, rem, SIMS)
        counts.append(c)
        if len(counts) == pl.SEARCH_CASES[name][0]:
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


def run_eager(name, rule, prior):
    """rp_search_step -> rp_rollout_eval -> rp_commit_eval on one engine."""
    import torch
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = pl.search_instance(name)
    eng = engine(name, sims=SIMS, move_rule=rule, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_playout_policy(*POLICY); eng.set_playout_landing(LAND)
    if prior != (0, 0, 0):
        eng.set_rollout_prior(*prior)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh[None], [area], episode_id=[eid])
    pi = torch.zeros((1, W * N), device="cuda"); v = torch.zeros(1, device="cuda")
    counts = []
    for _ in range(100000):
        if eng.search_step():
            eng.rollout_eval(v.data_ptr(), 1, K_SEARCH, pi_ptr=pi.data_ptr())
            eng.commit_eval(pi.data_ptr(), v.data_ptr())
        elif watch(eng, counts, pl.SEARCH_CASES[name][0]):
            break
    eng.check()
    tree = tree_as_dict(eng.dump_tree(0))
    eng.close()
    return counts, tree


def run_graph(name, rule, prior):
    """The captured wave of BatchedSelfPlay, one instance on one slot."""
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = pl.search_instance(name)
    game, args = _game_args(W, H, N, SIMS)
    sp = BatchedSelfPlay(game, None, args, games=1, groups=1, move_rule=rule, seed=SEED, tie_salt=SALT, evaluator="rollout", playouts=K_SEARCH,
                         use_graph=True, reclaim=False, playout_policy=POLICY, playout_landing=LAND, rollout_prior=prior)  # reclaim off: the oracle keeps every node
    assert sp.eng.playout_policy() == POLICY and sp.eng.playout_landing() == LAND and sp.eng.rollout_prior() == prior
    sp.start(wh[None], np.array([area], np.int32), buf, first_id=eid)
    counts = []
    for _ in range(100000):
        sp.step()
        if watch(sp.eng, counts, pl.SEARCH_CASES[name][0]):
            break
    assert sp.groups[0].graph is not None
    sp.eng.check()
    tree = tree_as_dict(sp.eng.dump_tree(0))
    sp.close()
    return counts, tree


def check_search(name, sample, prior):
    from resource_packing_self_play_amd import _lib
    rule = _lib.MOVE_SAMPLE if sample else _lib.MOVE_ARGMAX_FIRST
    want_counts, want_tree = oracle_search(name, sample, prior)
    runs = {"eager": run_eager(name, rule, prior), "graph": run_graph(name, rule, prior)}
    for how, (counts, tree) in runs.items():
        assert len(counts) == len(want_counts), how
        for k, (c, w) in enumerate(zip(counts, want_counts)):
            assert np.array_equal(c, w), "%s, %s: move %d" % (name, how, k)
        assert_trees_equal(tree, want_tree, "%s, %s" % (name, how))
    assert_trees_equal(runs["eager"][1], runs["graph"][1], name + ": eager against graph")
    return want_counts


@pytest.mark.parametrize("sample", [False, True], ids=["argmax_first", "sample"])
@pytest.mark.parametrize("name", list(pl.SEARCH_CASES))
def test_search_under_width2_landing2_matches_the_oracle(name, sample):
    check_search(name, sample, (0, 0, 0))


def test_search_with_the_rollout_prior_on_as_well_matches_the_oracle():
    check_search("10x10/8", True, pl.SEARCH_PRIOR)


# ---- 3. playout incumbents ---------------------------------------------------------------------------------------------------------------------
def test_playout_incumbents_replay_under_the_setting(monkeypatch):
    """The offer's winner is played again under the setting that scored it: every finished record is best_playout_ref's with the
    restatement's functions in rollout_ref's place, and its action list replays through solve.replay_rows to its board and score."""
    import test_gpu_best_playout as tb
    from resource_packing_self_play_amd import solve
    pl.under(monkeypatch, POLICY, LAND)
    W, H, bin_h, N, sims, games = br.SHAPES[1]
    wh = br.instances(W, bin_h, N, games)
    area = np.full(games, W * bin_h, np.int32)
    refs = [bp.episode(W, H, N, wh[g], int(area[g]), br.BUF, sims, bp.SAMPLE, br.SEED, br.SALT, g, bp.PLAYOUTS) for g in range(games)]
    eng = tb.make_engine(W, H, N, games, sims, tb.rules(bp.SAMPLE))
    eng.set_trace(True); eng.set_incumbent(True); eng.set_incumbent_playouts(True)
    eng.set_playout_policy(*POLICY); eng.set_playout_landing(LAND)
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
        if j >= 0:  # the restatement's playout j from the leaf reached after tree_moves actions: the action list is the scorer's
            _, leaf = solve.replay_rows(W, H, wh[g], got["action"][:tm])
            leaf_rem = np.ones(N, np.uint8); leaf_rem[[int(a) // W for a in got["action"][:tm]]] = 0
            trace = []
            mv, fb, _ = pl.playout_path(W, H, N, ev.unpack_board(leaf, W), leaf_rem, wh[g], br.SEED, g, j, trace=trace, policy=POLICY, land_pow=LAND)
            assert [t[3] for t in trace] == [int(a) for a in got["action"][tm:m]] and mv == m - tm, g
            assert np.array_equal(ev.pack_board(fb), got["board"]), g
            from_playouts += 1
    assert from_playouts >= 1, "no incumbent came from a playout"


# ---- 4. back to 0 ------------------------------------------------------------------------------------------------------------------------------
def test_zero_after_two_is_the_untouched_context():
    """Landing 2 and then 0: rollout_states, rollout_paths and a short episode's searches equal those of a context that never called the setter."""
    import torch
    from resource_packing_self_play_amd import _lib
    name, sims, K = "10x10/8", 16, 3
    W, H, N, _ = rr.GEOMETRIES[name]
    states = pl.gpu_states(name)
    rows, rem, wh, area, max_h, ids = state_arrays(states)
    runs = []
    for touch in (False, True):
        eng = engine(name, sims=sims, move_rule=_lib.MOVE_SAMPLE, stream=torch.cuda.current_stream().cuda_stream)
        landed = None
        if touch:
            eng.set_playout_landing(2)
            landed = eng.rollout_states(rows, rem, wh, area, max_h, rr.BUFFERS["mixed"], rr.ALPHA, K, episode_id=ids)
            eng.set_playout_landing(0)
        assert eng.playout_landing() == 0 and eng.playout_policy() == (0, 0)
        out = list(eng.rollout_states(rows, rem, wh, area, max_h, rr.BUFFERS["mixed"], rr.ALPHA, K, episode_id=ids))
        out += list(eng.rollout_paths(rows, rem, wh, K, episode_id=ids))
        if landed is not None:
            assert not np.array_equal(landed[3], out[3]), "the landing playouts ended on the uniform ones' boards"
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
    assert eng.playout_landing() == 0  # the default
    for x in (1, 2, 0, 1):
        eng.set_playout_landing(x)
        assert eng.playout_landing() == x
    for bad in (-1, 3):
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_playout_landing(bad)
        assert ei.value.code == _lib.ERR_ARG
        assert eng.playout_landing() == 1 and eng.playout_policy() == (0, 0)  # a refused call changes nothing
    eng.begin_episodes(wh[None], [area])
    assert eng.search_step() == 1  # the slot waits for its root's evaluation
    for x in (0, 1, 2):
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_playout_landing(x)
        assert ei.value.code == _lib.ERR_STATE and "middle of an episode" in str(ei.value)
    assert eng.playout_landing() == 1
    eng.close()


def test_python_api_and_refusals():
    from resource_packing_self_play_amd import solve
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    from test_gpu_packings import cnn_setup
    name = "10x10/8"
    W, H, N, _ = rr.GEOMETRIES[name]
    game, args = _game_args(W, H, N, 8)
    rng = np.random.default_rng(6)
    wh = np.stack([rr.make_items(name, rng)[0] for _ in range(3)])
    board0, rem0 = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    for bad in (3, -1, True, 1.0, "2"):
        with pytest.raises(ValueError):
            solve.random_scores(game, item_wh=wh, playouts=2, playout_landing=bad)
        with pytest.raises(ValueError):
            solve.pack(game, None, args, item_wh=wh, evaluator="rollout", playouts=2, playout_landing=bad)
        with pytest.raises(ValueError):
            BatchedSelfPlay(game, None, args, games=2, evaluator="rollout", playout_landing=bad)
    cnn_game, nnet, cnn_args = cnn_setup(W, H, N, 8)
    for kw in (dict(playout_landing=2), dict(playout_landing=1, evaluator="cnn")):  # the CNN runs no playouts
        with pytest.raises(ValueError):
            solve.pack(cnn_game, nnet, cnn_args, item_wh=wh, **kw)
        with pytest.raises(ValueError):
            BatchedSelfPlay(cnn_game, nnet, cnn_args, games=2, **kw)
    sp = BatchedSelfPlay(game, None, args, games=2, evaluator="rollout", playouts=2, record_packings=True, playout_landing=1)
    try:
        for other in (0, 2):
            with pytest.raises(RuntimeError):
                solve.pack(game, None, args, item_wh=wh, driver=sp, playout_landing=other)
    finally:
        sp.close()
    # the scores are the restatement's
    scores = solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED, playout_policy="width2", playout_landing=2)
    want = [[pl.playout(W, H, N, board0, rem0, wh[i], int(wh[i, :, 0].astype(int) @ wh[i, :, 1]), [], SEED, SALT, i, j, policy=(2, 0), land_pow=2)[1]
             for j in range(3)] for i in range(3)]
    assert np.array_equal(scores, np.array(want))
    assert np.array_equal(solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED, playout_landing=0), solve.random_scores(game, item_wh=wh, playouts=3, seed=SEED))
    # pack under the setting plays the oracle's episodes with the restatement as evaluator, and returns complete Packings
    buf = scores.reshape(-1)
    packs = solve.pack(game, None, args, item_wh=wh, evaluator="rollout", playouts=3, rewards_list=buf, seed=SEED, tie_salt=SALT, playout_policy="width2",
                       playout_landing=2, best=True, playout_incumbents=True)
    assert len(packs) == 3
    for i, p in enumerate(packs):
        m = pl.oracle(W, H, N, wh[i], W * H, buf, SEED, SALT, i, 3, (2, 0), 2)
        actions, _, o, s = m.play_episode(8, policy=0, want_counts=False)
        m.close()
        assert list(p.played.actions) == [int(x) for x in actions] and (p.played.outcome, p.played.score) == (o, s), i
        assert p.score >= p.played.score
        p.layout()
