"""GPU parity: the HIP tree search through the C ABI against (a) golden episodes captured from the
reference's MCTS_bpp.MCTS and (b) the CPU oracle on freshly generated games.  Everything is compared
bit for bit: visit counts per move, chosen placements, every node's Ns / Es and every edge's P, Nsa, Q."""
import glob
import os

import numpy as np
import pytest

import evaluators as ev
import oracle_lib as orc
from engine_util import assert_trees_equal, fixture_tree, host_evaluator, planes_from_state, run_until_idle, tree_as_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MCTS_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mcts_*.npz")))


def make_engine(*a, **kw):
    from resource_packing_self_play_amd._lib import Engine
    return Engine(*a, **kw)


@pytest.mark.parametrize("path", MCTS_FILES, ids=[os.path.basename(p)[5:-4] for p in MCTS_FILES])
def test_episode_matches_reference_golden(path):
    from resource_packing_self_play_amd import _lib
    d = np.load(path)
    W, H, N, sims = int(d["W"]), int(d["H"]), int(d["N"]), int(d["sims"])
    kind, salt = str(d["kind"]), int(d["salt"])
    eng = make_engine(W, H, N, 1, sims, cpuct=float(d["cpuct"]), alpha=float(d["alpha"]), move_rule=_lib.MOVE_EXTERNAL, tie_salt=salt)
    eng.set_rank_buffer(d["buf"])
    wh = np.stack([d["item_w"], d["item_h"]], axis=1)[None]
    eng.begin_episodes(wh, [int(d["total_area"])])
    evaluate = host_evaluator(lambda s: kind, W * N, lambda s: salt)
    evals = 0
    for mv, action in enumerate(d["actions"]):
        evals += run_until_idle(eng, evaluate)
        ph, sd, moves, _ = eng.status()
        assert ph[0] == _lib.PHASE_MOVE_READY and sd[0] == sims and moves[0] == mv
        counts = eng.root_counts()[0]
        assert np.array_equal(counts, d["counts"][mv]), "visit counts differ at move %d" % mv
        ended, score = eng.advance_roots([int(action)])
        if mv + 1 < len(d["actions"]):
            assert ended[0] == 0
    assert ended[0] == int(d["outcome"]) and score[0] == float(d["score"])
    assert evals == int(d["evals"])
    assert_trees_equal(tree_as_dict(eng.dump_tree(0)), fixture_tree(d), os.path.basename(path))
    c = eng.counters()
    assert c["expansions"] == int(d["evals"]) and c["simulations"] == sims * len(d["actions"])
    eng.close()


CASES = [  # W, H, N, sims, games, kind, rule
    (10, 10, 8, 50, 48, "hashed", "argmax"),
    (10, 10, 8, 64, 40, "sparse", "sample"),
    (10, 10, 8, 30, 32, "peaked", "sample"),
    (20, 20, 32, 24, 12, "hashed", "sample"),
    (15, 15, 10, 40, 16, "uniform", "argmax"),
    (33, 12, 9, 30, 8, "hashed", "sample"),  # 64-bit rows
    (50, 50, 128, 10, 3, "peaked", "argmax"),
    # nodes on both sides of the 64-legal-move boundary (one-pass scoring below it, cached best unvisited move + rescans above it)
    (16, 16, 14, 60, 10, "peaked", "sample"),
    (40, 30, 60, 16, 4, "uniform", "argmax"),  # equal priors everywhere: every first visit takes the lowest unvisited action and rescans
    (24, 24, 40, 40, 6, "sparse", "sample"),   # zeros among the priors and the all-zero fallback on nodes with > 64 legal moves
    # 8 192 actions, 64-bit rows, N > 64: the smallest board whose legal-move staging passes the default 64 KB of LDS (k_set_roots, k_search, k_moves)
    (64, 4, 128, 6, 2, "hashed", "sample"),
]


def gen_items(rng, W, H, N):
    """guillotine split of the W x H rectangle into N items, like ItemsGenerator (BinPackingGame.py:257-285)."""
    items = [(W, H)]
    while len(items) < N:
        k = int(rng.integers(len(items))); w, h = items[k]
        if rng.integers(2) == 0:
            if w == 1: continue
            c = int(rng.integers(1, w)); items.pop(k); items += [(c, h), (w - c, h)]
        else:
            if h == 1: continue
            c = int(rng.integers(1, h)); items.pop(k); items += [(w, c), (w, h - c)]
    return np.array(items, np.uint8)


@pytest.mark.parametrize("W,H,N,sims,games,kind,rule", CASES)
def test_self_play_matches_oracle(W, H, N, sims, games, kind, rule):
    """Whole episodes with the engine's own move rules (auto moves on device) vs the oracle playing the
    same instances: every action, outcome, score, and the complete final tree of every game."""
    from resource_packing_self_play_amd import _lib
    rng = np.random.default_rng(W * 7 + N + sims)
    A = W * N
    seed, salt = 1234 + sims, 99
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(games)])
    area = np.full(games, W * H, np.int32)
    ratios = [a / b for a in range(1, H + 1) for b in range(a, H + 1)]
    buf = rng.choice(ratios, size=60)
    move_rule = _lib.MOVE_ARGMAX_FIRST if rule == "argmax" else _lib.MOVE_SAMPLE
    eng = make_engine(W, H, N, games, sims, cpuct=1.0, alpha=0.75, move_rule=move_rule, seed=seed, tie_salt=salt,
                      edge_cap=2_000_000 if W == 50 else 0)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh, area, episode_id=np.arange(games) + 1000)
    evaluate = host_evaluator(lambda s: kind, A, lambda s: salt)
    run_until_idle(eng, evaluate)
    ph, _, moves, _ = eng.status()
    assert (ph == _lib.PHASE_EPISODE_DONE).all()
    ids, outcome, score, nmoves = eng.pop_finished()
    fin = {int(i): (int(o), float(s), int(m)) for i, o, s, m in zip(ids, outcome, score, nmoves)}
    assert len(fin) == games
    stats = dict.fromkeys(("expansions", "searches", "terminal_returns", "path_edges", "sum_valid_select", "sum_valid_leaf", "transposition_hits", "nodes"), 0)
    for g in range(games):
        m = orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval(kind, ev.pack_board(b), r, A, salt),
                           lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))
        m.begin_episode(wh[g, :, 0], wh[g, :, 1], W * H, buf)
        actions, _, o, s = m.play_episode(sims, policy=0 if rule == "argmax" else 1, seed=seed, episode_id=1000 + g, want_counts=False)
        assert fin[1000 + g] == (o, s, len(actions)), g
        assert moves[g] == len(actions)
        assert_trees_equal(tree_as_dict(eng.dump_tree(g)), m.dump(), "game %d" % g)
        for k, v in m.stats().items():
            stats[k] += v
        m.close()
    c = eng.counters()
    assert c["simulations"] == stats["searches"] and c["expansions"] == stats["expansions"]
    assert c["terminal_returns"] == stats["terminal_returns"] and c["path_edges"] == stats["path_edges"]
    assert c["sum_valid_select"] == stats["sum_valid_select"] and c["sum_valid_leaf"] == stats["sum_valid_leaf"]
    assert c["nodes"] == stats["nodes"] and c["transposition_links"] == stats["transposition_hits"]
    assert c["episodes"] == games
    eng.close()


def test_set_roots_keeps_the_tree_like_getActionProb():
    """MCTS.getActionProb on successive states of one MCTS object (CoachBPP.py:74-78): the engine is re-rooted with
    rp_set_roots and must give the same counts as the oracle whose dicts persist."""
    from resource_packing_self_play_amd import _lib
    W, H, N, sims = 10, 10, 8, 40
    A = W * N
    rng = np.random.default_rng(5)
    wh = gen_items(rng, W, H, N)
    eng = make_engine(W, H, N, 1, sims, move_rule=_lib.MOVE_EXTERNAL, tie_salt=3)
    eng.set_rank_buffer([0.9, 0.8, 1.0])
    eng.begin_episodes(wh[None], [W * H])
    m = orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval("hashed", ev.pack_board(b), r, A, 3), lambda b, r: ev.tie_value(ev.pack_board(b), r, 3))
    m.begin_episode(wh[:, 0], wh[:, 1], W * H, [0.9, 0.8, 1.0])
    evaluate = host_evaluator(lambda s: "hashed", A, lambda s: 3)
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    for step in range(5):
        eng.set_roots(ev.pack_board(board)[None], rem[None])
        run_until_idle(eng, evaluate)
        counts = eng.root_counts()[0]
        want = m.action_counts(board, rem, sims)
        assert np.array_equal(counts, want), step
        valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        if n == 0:
            break
        a = int(rng.choice(np.nonzero(valid)[0]))  # any legal move, also one the search never visited
        _, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, a)
    assert_trees_equal(tree_as_dict(eng.dump_tree(0)), m.dump())
    eng.close(); m.close()


def test_leaf_planes_match_getBinItem():
    import torch
    from resource_packing_self_play_amd import _lib
    for (W, H, N) in [(10, 10, 8), (20, 20, 32), (33, 12, 9)]:
        games, sims = 16, 6
        rng = np.random.default_rng(N)
        wh = np.stack([gen_items(rng, W, H, N) for _ in range(games)])
        eng = make_engine(W, H, N, games, sims, move_rule=_lib.MOVE_ARGMAX_FIRST, stream=torch.cuda.current_stream().cuda_stream)
        eng.begin_episodes(wh, np.full(games, W * H, np.int32))
        evaluate = host_evaluator(lambda s: "hashed", W * N, lambda s: 0)
        buf = torch.full((games, N + 1, H, W), -7.0, device="cuda")
        for step in range(30):
            n = eng.search_step()
            if n == 0:
                continue  # between two moves
            eng.leaf_planes(buf.data_ptr(), games)
            rows, rem, slots = eng.leaf_states(n)
            got = buf.cpu().numpy()
            for b in range(n):
                want = planes_from_state(rows[b], rem[b], wh[slots[b]], W, H)
                assert np.array_equal(got[b], want), (W, step, b)
            pi, v = evaluate(rows, rem, slots)
            eng.commit_eval_host(pi, v)
        eng.close()


def test_capacity_overflow_is_reported():
    from resource_packing_self_play_amd import _lib
    W, H, N = 10, 10, 8
    rng = np.random.default_rng(0)
    wh = gen_items(rng, W, H, N)
    eng = make_engine(W, H, N, 1, 50, move_rule=_lib.MOVE_ARGMAX_FIRST, node_cap=12)
    eng.begin_episodes(wh[None], [W * H])
    evaluate = host_evaluator(lambda s: "uniform", W * N, lambda s: 0)
    with pytest.raises(_lib.EngineError) as ei:
        run_until_idle(eng, evaluate)
    assert ei.value.code == _lib.ERR_CAPACITY
    eng.close()


def _play_pool(W, H, N, sims, wh, games, step_cap, kind, salt, seed, buf):
    from resource_packing_self_play_amd import _lib
    eng = make_engine(W, H, N, games, sims, move_rule=_lib.MOVE_SAMPLE, seed=seed, tie_salt=salt, auto_restart=1)
    eng.set_step_cap(step_cap)
    eng.set_rank_buffer(buf)
    area = np.full(len(wh), W * H, np.int32)
    eng._ck(eng.L.rp_set_instance_pool(eng.h, len(wh), _lib._ptr(np.ascontiguousarray(wh)), _lib._ptr(area), 500))
    eng._ck(eng.L.rp_begin_pool(eng.h))
    run_until_idle(eng, host_evaluator(lambda s: kind, W * N, lambda s: salt))
    ids, outcome, score, moves = eng.pop_finished()
    order = np.argsort(ids)
    c = eng.counters()
    eng.close()
    return ids[order], outcome[order], score[order], moves[order], c


def test_results_do_not_depend_on_slot_count_or_step_cap():
    """Scheduling independence: the same pool of instances through 24, 7 or 5 slots, with or without the per-launch simulation
    cap, finishes with identical episodes and identical engine counters; a sample is checked against the oracle."""
    W, H, N, sims = 20, 20, 32, 48
    rng = np.random.default_rng(77)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(24)])
    buf = rng.uniform(0.7, 1.0, 50)
    runs = [_play_pool(W, H, N, sims, wh, g, cap, "hashed", 11, 4242, buf) for g, cap in ((24, 0), (7, 3), (5, 1))]
    for r in runs[1:]:
        for a, b in zip(runs[0][:4], r[:4]):
            assert np.array_equal(a, b)
        for k in ("simulations", "expansions", "terminal_returns", "path_edges", "sum_valid_select", "sum_valid_leaf", "nodes", "moves", "episodes"):
            assert runs[0][4][k] == r[4][k], k
    assert list(runs[0][0]) == list(range(500, 524))
    A = W * N
    for g in (0, 9, 23):
        m = orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval("hashed", ev.pack_board(b), r, A, 11), lambda b, r: ev.tie_value(ev.pack_board(b), r, 11))
        m.begin_episode(wh[g, :, 0], wh[g, :, 1], W * H, buf)
        actions, _, o, s = m.play_episode(sims, policy=1, seed=4242, episode_id=500 + g, want_counts=False)
        assert (runs[0][1][g], runs[0][2][g], runs[0][3][g]) == (o, s, len(actions))
        m.close()


def test_staged_pool_and_advance_kernels_beyond_64k_lds():
    """k_pool_begin and k_advance at 8 192 actions, where the legal-move staging passes the default 64 KB of LDS (the CASES row of
    this board runs the other three staged kernels): (a) a pool's episodes and (b) an externally moved episode against the oracle."""
    from resource_packing_self_play_amd import _lib
    W, H, N, sims = 64, 4, 128, 6
    A, salt, seed = W * N, 17, 777
    rng = np.random.default_rng(64)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(3)])
    buf = rng.uniform(0.7, 1.0, 50)

    def oracle():
        return orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval("hashed", ev.pack_board(b), r, A, salt), lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))

    ids, outcome, score, moves, c = _play_pool(W, H, N, sims, wh, 2, 0, "hashed", salt, seed, buf)  # (a) k_pool_begin
    assert list(ids) == [500, 501, 502]
    stats = dict.fromkeys(("searches", "expansions", "nodes"), 0)
    for g in range(3):
        m = oracle()
        m.begin_episode(wh[g, :, 0], wh[g, :, 1], W * H, buf)
        actions, _, o, s = m.play_episode(sims, policy=1, seed=seed, episode_id=500 + g, want_counts=False)
        assert (outcome[g], score[g], moves[g]) == (o, s, len(actions)), g
        for k in stats:
            stats[k] += m.stats()[k]
        m.close()
    assert (c["simulations"], c["expansions"], c["nodes"], c["episodes"]) == (stats["searches"], stats["expansions"], stats["nodes"], 3)

    eng = make_engine(W, H, N, 1, sims, cpuct=1.0, alpha=0.75, move_rule=_lib.MOVE_EXTERNAL, tie_salt=salt)  # (b) k_advance
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh[:1], [W * H])
    evaluate = host_evaluator(lambda s: "hashed", A, lambda s: salt)
    played, ended = [], np.zeros(1, np.int32)
    while ended[0] == 0 and len(played) <= N:
        run_until_idle(eng, evaluate)
        played.append(int(np.argmax(eng.root_counts()[0])))  # the first action with the highest count
        ended, sc = eng.advance_roots(played[-1:])
    m = oracle()
    m.begin_episode(wh[0, :, 0], wh[0, :, 1], W * H, buf)
    actions, _, o, s = m.play_episode(sims, policy=0, want_counts=False)
    assert played == list(actions)
    assert (ended[0], sc[0]) == (o, s)
    assert_trees_equal(tree_as_dict(eng.dump_tree(0)), m.dump())
    eng.close(); m.close()


@pytest.mark.parametrize("cfg,W,H,N,sims,games,min_nodes", [("c3", 20, 20, 32, 400, 4, 3000), ("c4", 20, 20, 32, 100, 4, 800), ("c5", 50, 50, 128, 200, 1, 5000)])
def test_full_size_episodes_match_oracle(cfg, W, H, N, sims, games, min_nodes):
    """BASELINE configs[2] (20x20 / 32 items / 400 sims) and configs[3] (the same board at 100 sims) at full size for a few games,
    and configs[4]'s board (50x50, 128 items: 64-bit rows, 6 400 actions, 129 levels) at 200 sims per move for one game -- the
    default node_cap / arena sizing of a deep tree: whole episodes with sampled moves, every action, the outcome and the
    complete tree of each game against the oracle.  (c5's own 800 sims per move differ only in the loop count; the oracle needs
    ~4x as long.)"""
    from resource_packing_self_play_amd import _lib
    A = W * N
    rng = np.random.default_rng(2020 + sims)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(games)])
    buf = rng.uniform(0.8, 1.0, 100)
    eng = make_engine(W, H, N, games, sims, move_rule=_lib.MOVE_SAMPLE, seed=9, tie_salt=5)
    eng.set_step_cap(16)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh, np.full(games, W * H, np.int32), episode_id=np.arange(games) + 70)
    run_until_idle(eng, host_evaluator(lambda s: "peaked", A, lambda s: 5))
    ids, outcome, score, moves = eng.pop_finished()
    fin = {int(i): (int(o), float(s), int(mv)) for i, o, s, mv in zip(ids, outcome, score, moves)}
    for g in range(games):
        m = orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval("peaked", ev.pack_board(b), r, A, 5), lambda b, r: ev.tie_value(ev.pack_board(b), r, 5))
        m.begin_episode(wh[g, :, 0], wh[g, :, 1], W * H, buf)
        actions, _, o, s = m.play_episode(sims, policy=1, seed=9, episode_id=70 + g, want_counts=False)
        assert fin[70 + g] == (o, s, len(actions)), g
        tree = tree_as_dict(eng.dump_tree(g))
        assert len(tree) > min_nodes, len(tree)
        assert_trees_equal(tree, m.dump(), "%s game %d" % (cfg, g))
        m.close()
    pk = eng.arena_peak()
    print("%s: arena peak per slot %s" % (cfg, pk))
    eng.close()


def test_reclaiming_dead_levels_changes_nothing():
    """DP::reclaim recycles the arena chunks of a level once the root has moved past it.  Same pool, with and without it, in
    arenas that would overflow without recycling: identical episodes and counters; the peak arena use drops."""
    from resource_packing_self_play_amd import _lib
    W, H, N, sims = 20, 20, 32, 64
    rng = np.random.default_rng(31)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(12)])
    buf = rng.uniform(0.7, 1.0, 50)
    area = np.full(len(wh), W * H, np.int32)
    out = {}
    for reclaim in (0, 1):
        eng = make_engine(W, H, N, 6, sims, move_rule=_lib.MOVE_SAMPLE, seed=77, tie_salt=3, auto_restart=1, reclaim=reclaim)
        eng.set_step_cap(4)
        eng.set_rank_buffer(buf)
        eng._ck(eng.L.rp_set_instance_pool(eng.h, len(wh), _lib._ptr(np.ascontiguousarray(wh)), _lib._ptr(area), 0))
        eng._ck(eng.L.rp_begin_pool(eng.h))
        run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: 3))
        ids, outcome, score, moves = eng.pop_finished()
        order = np.argsort(ids)
        out[reclaim] = (ids[order], outcome[order], score[order], moves[order], eng.counters(), eng.arena_peak())
        eng.close()
    for a, b in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(a, b)
    for k in ("simulations", "expansions", "terminal_returns", "path_edges", "sum_valid_select", "sum_valid_leaf", "nodes", "visited_new"):
        assert out[0][4][k] == out[1][4][k], k
    print("arena peak without / with reclaim:", out[0][5], out[1][5])
    assert out[1][5]["prior_chunks"] < out[0][5]["prior_chunks"]
    # a tight arena only works with recycling
    tight = dict(edge_cap=out[1][5]["prior_chunks"] * 4096 + 4096, vis_cap=out[1][5]["visited_chunks"] * 1024 + 1024)
    eng = make_engine(W, H, N, 6, sims, move_rule=_lib.MOVE_SAMPLE, seed=77, tie_salt=3, auto_restart=1, reclaim=1, **tight)
    eng.set_rank_buffer(buf)
    eng._ck(eng.L.rp_set_instance_pool(eng.h, len(wh), _lib._ptr(np.ascontiguousarray(wh)), _lib._ptr(area), 0))
    eng._ck(eng.L.rp_begin_pool(eng.h))
    run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: 3))
    ids, outcome, score, moves = eng.pop_finished()
    assert np.array_equal(outcome[np.argsort(ids)], out[0][1])
    eng.close()
    eng = make_engine(W, H, N, 6, sims, move_rule=_lib.MOVE_SAMPLE, seed=77, tie_salt=3, auto_restart=1, reclaim=0, **tight)
    eng.set_rank_buffer(buf)
    eng._ck(eng.L.rp_set_instance_pool(eng.h, len(wh), _lib._ptr(np.ascontiguousarray(wh)), _lib._ptr(area), 0))
    eng._ck(eng.L.rp_begin_pool(eng.h))
    with pytest.raises(_lib.EngineError):
        run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: 3))
    eng.close()


@pytest.mark.timeout(1200)
def test_c5_at_800_sims_matches_oracle_digest():
    """BASELINE configs[4] at its OWN depth: 50x50 bin, 128 items, numMCTSSims = 800 per move (MCTS_bpp.py:37-38), one whole game with the
    engine's DEFAULT node_cap (800 * 129 + 2) and arena sizing, sampled moves.  The oracle needs ~3 minutes and ~10 GB for this
    game, so its answer is a committed fixture (tests/golden/make_c5_digest.py, generated with the pinned C oracle in the build
    container): number of moves, outcome, score, the oracle's counters, the node count, and SHA-256 digests -- of the whole tree and
    per level -- over every node's (key, Es, Ns) and every legal move's (action, P, Nsa, Q, kind)."""
    import json
    from engine_util import tree_digest
    from resource_packing_self_play_amd import _lib
    f = json.load(open(os.path.join(GOLDEN, "mcts_c5_800_digest.json")))
    W, H, N, sims, A = f["W"], f["H"], f["N"], f["sims"], f["W"] * f["N"]
    assert (W, H, N, sims) == (50, 50, 128, 800)
    wh = np.array(f["item_wh"], np.uint8)
    eng = make_engine(W, H, N, 1, sims, cpuct=f["cpuct"], alpha=f["alpha"], move_rule=_lib.MOVE_SAMPLE, seed=f["seed"], tie_salt=f["salt"])
    eng.set_step_cap(16)
    eng.set_rank_buffer(np.array(f["buf"]))
    eng.begin_episodes(wh[None], [W * H], episode_id=[f["episode_id"]])
    run_until_idle(eng, host_evaluator(lambda s: f["kind"], A, lambda s: f["salt"]))
    ids, outcome, score, moves = eng.pop_finished()
    assert (int(ids[0]), int(outcome[0]), float(score[0]), int(moves[0])) == (f["episode_id"], f["outcome"], f["score"], len(f["actions"]))
    c, st = eng.counters(), f["stats"]
    assert c["simulations"] == st["searches"] and c["expansions"] == st["expansions"] and c["terminal_returns"] == st["terminal_returns"]
    assert c["path_edges"] == st["path_edges"] and c["sum_valid_select"] == st["sum_valid_select"] and c["sum_valid_leaf"] == st["sum_valid_leaf"]
    assert c["nodes"] == st["nodes"] == f["n_nodes"] and c["transposition_links"] == st["transposition_hits"]
    tree = tree_as_dict(eng.dump_tree(0))
    assert len(tree) == f["n_nodes"]
    digest, levels = tree_digest(tree, N)
    bad = [lv for lv, (cnt, dg) in levels.items() if [cnt, dg] != f["levels"].get(str(lv))]
    assert not bad and len(levels) == len(f["levels"]), "levels (items placed) whose nodes differ from the oracle's: %s" % bad[:10]
    assert digest == f["tree_sha256"]
    print("c5 at 800 sims: %d nodes, %d moves, arena peak %s" % (len(tree), int(moves[0]), eng.arena_peak()))
    eng.close()


@pytest.mark.parametrize("W,H,N", [(10, 10, 8), (20, 20, 32), (33, 12, 9)])
def test_commit_from_logits_equals_commit_from_softmax(W, H, N):
    """rp_commit_eval_logits (the softmax of NNet.predict, NNet.py:81-85, taken inside the commit kernel) against rp_commit_eval fed
    torch.softmax of the same logits: the same legal moves, expansion state and value backup; every prior P = pi / sum within float32
    rounding of the softmax (1e-6 relative: the two differ in the order of the float32 sum); the uniform fallback (MCTS_bpp.py:93-100) cannot
    be reached through a softmax and is not exercised here.  Action spaces beyond the kernel's LDS row buffer are refused."""
    import torch
    from resource_packing_self_play_amd import _lib
    games, A = 48, W * N
    rng = np.random.default_rng(W + N)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(games)])
    torch.manual_seed(W)
    logits = (torch.randn(games, A, device="cuda") * 4.0).contiguous()
    logits[3] = 0.0  # a flat row
    logits[5, : A // 2] = -60.0  # probabilities that underflow to denormals / zero
    v = torch.tanh(torch.randn(games, device="cuda")).contiguous()
    trees = []
    for mode in ("softmax", "logits"):
        eng = make_engine(W, H, N, games, 4, move_rule=_lib.MOVE_EXTERNAL, stream=torch.cuda.current_stream().cuda_stream)
        eng.begin_episodes(wh, np.full(games, W * H, np.int32))
        assert eng.search_step() == games  # every root waits for the evaluator, row b = slot b
        if mode == "softmax":
            pi = torch.softmax(logits, dim=1).contiguous()
            eng.commit_eval(pi.data_ptr(), v.data_ptr())
        else:
            eng.commit_eval_logits(logits.data_ptr(), v.data_ptr())
        torch.cuda.synchronize()
        ph, sd, _, _ = eng.status()
        assert (ph == _lib.PHASE_RUNNING).all() and (sd == 1).all()
        trees.append([tree_as_dict(eng.dump_tree(g)) for g in range(games)])
        eng.close()
    worst = 0.0
    for g in range(games):
        a, b = trees[0][g], trees[1][g]
        assert a.keys() == b.keys() and len(a) == 1
        for key in a:
            ra, rb = a[key], b[key]
            assert ra["expanded"] == rb["expanded"] == 1 and ra["ns"] == rb["ns"] == 0 and np.array_equal(ra["actions"], rb["actions"])
            assert abs(ra["p"].sum() - 1.0) < 1e-12 and abs(rb["p"].sum() - 1.0) < 1e-12
            rel = np.abs(ra["p"] - rb["p"]) / np.maximum(ra["p"], 1e-30)
            worst = max(worst, float(rel[ra["p"] > 1e-30].max()))
    print("%dx%d/%d: max relative difference of a prior, logits path vs torch.softmax path: %.2e" % (W, H, N, worst))
    assert worst < 2e-6
    big = make_engine(50, 50, 128, 1, 1, move_rule=_lib.MOVE_EXTERNAL)
    with pytest.raises(_lib.EngineError):
        big.commit_eval_logits(logits.data_ptr(), v.data_ptr())
    big.close()
