"""GPU parity of the placement trace (rp_set_trace / rp_pop_finished_packings), solve.pack() and CoachBPP's arena and gate.
Everything is compared bit for bit: the trace against the CPU oracle's episodes replayed through its own rules, against the
capture of the reference's CoachBPP.learn, and against the engine's golden-pinned stateless rules on the production path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import evaluators as ev
import oracle_lib as orc
from engine_util import host_evaluator, run_until_idle
from test_gpu_mcts import gen_items

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ALPHA = 0.75


# ---- the oracle's side ------------------------------------------------------------------------------------------------------
def host_draw(counts, seed, episode, move):
    """RP_MOVE_ARGMAX_DRAW (rp_engine.h): entry umulhi(x, m) of the m most-visited actions in ascending order."""
    best = np.flatnonzero(counts == counts.max())
    x = ev.splitmix64(ev.splitmix64(ev.splitmix64(seed) ^ int(episode)) ^ int(move))
    return int(best[(x * len(best)) >> 64])


def oracle_episode(W, H, N, wh, buf, kind, salt, sims, rule, seed, eid):
    """-> (actions, outcome, score) of the oracle's MCTS playing one instance under the engine's move rule `rule`."""
    from resource_packing_self_play_amd import _lib
    A = W * N
    m = orc.OracleMCTS(W, H, N, 1.0, ALPHA, lambda b, r: ev.table_eval(kind, ev.pack_board(b), r, A, salt), lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))
    m.begin_episode(wh[:, 0], wh[:, 1], W * H, buf)
    if rule in (_lib.MOVE_ARGMAX_FIRST, _lib.MOVE_SAMPLE):
        actions, _, o, s = m.play_episode(sims, policy=0 if rule == _lib.MOVE_ARGMAX_FIRST else 1, seed=seed, episode_id=eid, want_counts=False)
        m.close()
        return [int(a) for a in actions], o, s
    # the oracle has no draw rule: its counts move by move (one MCTS object, the tree is kept as in orc_play_episode), the documented draw
    C = orc.C
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    bufa = np.ascontiguousarray(buf, dtype=np.float64)
    actions = []
    while True:
        counts = m.action_counts(board, rem, sims)
        assert counts.max() > 0
        a = host_draw(counts, seed, eid, len(actions))
        actions.append(a)
        rc, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, a)
        assert rc == 0
        r = C.c_double()
        iw, ih = np.ascontiguousarray(wh[:, 0]), np.ascontiguousarray(wh[:, 1])
        e = orc.lib().orc_game_ended(W, H, N, orc._p8(board), orc._p8(iw), orc._p8(ih), orc._p8(rem), W * H, int(ih.max()),
                                     bufa.ctypes.data_as(C.POINTER(C.c_double)), len(bufa), ALPHA, C.byref(r))
        if e != 0:
            if e == 2:  # ORC_TIE
                e = ev.tie_value(ev.pack_board(board), rem, salt)
            m.close()
            return actions, int(e), r.value


def oracle_replay(W, H, N, wh, actions):
    """The oracle's rules over the actions -> (rows mask of every move, final row masks)."""
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    masks = []
    for a in actions:
        rc, nb, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, int(a))
        assert rc == 0
        masks.append(sum(1 << int(r) for r in np.flatnonzero(ev.pack_board(nb) != ev.pack_board(board))))
        board = nb
    return np.array(masks, np.uint64), ev.pack_board(board)


def kind_of_slot(s):
    return "hashed" if s % 2 == 0 else "uniform"  # uniform priors: every count ties


def records(eng):
    ids, oc, sc, mv, act, rows, board = eng.pop_finished(packings=True)
    return {int(i): (int(o), float(s), int(m), act[k], rows[k], board[k]) for k, (i, o, s, m) in enumerate(zip(ids, oc, sc, mv))}


def check_record(rec, W, H, N, wh, want_actions, want_outcome, want_score, where):
    o, s, m, act, rows, board = rec
    assert m == len(want_actions) and [int(a) for a in act[:m]] == list(want_actions), where
    masks, final = oracle_replay(W, H, N, wh, want_actions)
    assert np.array_equal(rows[:m], masks), where
    assert not act[m:].any() and not rows[m:].any(), where  # entries past the episode's moves are zero
    assert np.array_equal(board, final), where
    assert (o, s) == (want_outcome, want_score), where


SHAPES = [(10, 10, 8, 30, 6), (15, 15, 10, 30, 6), (20, 20, 32, 20, 4), (50, 50, 128, 6, 1)]  # W, H, N, sims, games


def setup_games(W, H, N, games):
    rng = np.random.default_rng(W * 31 + N)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(games)])
    ratios = [a / b for a in range(1, H + 1) for b in range(a, H + 1)]
    return wh, rng.choice(ratios, size=40)


@pytest.mark.parametrize("W,H,N,sims,games", SHAPES)
@pytest.mark.parametrize("rule", ["sample", "argmax_first", "argmax_draw"])
def test_trace_matches_the_oracle(rule, W, H, N, sims, games):
    from resource_packing_self_play_amd import _lib
    rule = dict(sample=_lib.MOVE_SAMPLE, argmax_first=_lib.MOVE_ARGMAX_FIRST, argmax_draw=_lib.MOVE_ARGMAX_DRAW)[rule]
    wh, buf = setup_games(W, H, N, games)
    seed, salt = 4321, 17
    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=ALPHA, move_rule=rule, seed=seed, tie_salt=salt, edge_cap=2_000_000 if W == 50 else 0)
    bytes_off = eng.device_bytes
    eng.set_trace(True)
    fin_cap = max(4 * games, 1024)
    assert eng.device_bytes - bytes_off == fin_cap * (N * 10 + H * 8) + games * N * 10  # the documented cost, nothing before the switch
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh, np.full(games, W * H, np.int32), episode_id=np.arange(games) + 300)
    run_until_idle(eng, host_evaluator(kind_of_slot, W * N, lambda s: salt))
    got = records(eng)
    assert sorted(got) == list(range(300, 300 + games))
    for g in range(games):
        actions, o, s = oracle_episode(W, H, N, wh[g], buf, kind_of_slot(g), salt, sims, rule, seed, 300 + g)
        check_record(got[300 + g], W, H, N, wh[g], actions, o, s, "game %d" % g)
    eng.close()


@pytest.mark.parametrize("W,H,N,sims,games", SHAPES)
def test_trace_of_external_moves(W, H, N, sims, games):
    """RP_MOVE_EXTERNAL: the host plays the oracle's (sampled) actions through rp_advance_roots."""
    from resource_packing_self_play_amd import _lib
    wh, buf = setup_games(W, H, N, games)
    seed, salt = 99, 5
    want = [oracle_episode(W, H, N, wh[g], buf, kind_of_slot(g), salt, sims, _lib.MOVE_SAMPLE, seed, 40 + g) for g in range(games)]
    eng = _lib.Engine(W, H, N, games, sims, cpuct=1.0, alpha=ALPHA, move_rule=_lib.MOVE_EXTERNAL, seed=seed, tie_salt=salt, edge_cap=2_000_000 if W == 50 else 0)
    eng.set_trace(True)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh, np.full(games, W * H, np.int32), episode_id=np.arange(games) + 40)
    evaluate = host_evaluator(kind_of_slot, W * N, lambda s: salt)
    for mv in range(max(len(w[0]) for w in want)):
        run_until_idle(eng, evaluate)
        for g in range(games):
            if mv < len(want[g][0]):
                ended, score = eng.advance_roots([want[g][0][mv]], first=g)
                assert (ended[0] != 0) == (mv + 1 == len(want[g][0]))
    got = records(eng)
    assert sorted(got) == list(range(40, 40 + games))
    for g in range(games):
        check_record(got[40 + g], W, H, N, wh[g], *want[g], "game %d" % g)
    eng.close()


def test_trace_against_the_reference_capture(tmp_path):
    """The episodes of tests/golden/coach_c1.npz replayed as test_gpu_coach.py replays them, with the trace on: the board after move m
    is the state the reference recorded for move m + 1, and the score is the reference's."""
    from resource_packing_self_play_amd import _lib
    from test_gpu_coach import make_coach
    f = np.load(os.path.join(GOLDEN, "coach_c1.npz"))
    E = int(f["numEps"])
    coach, args = make_coach(f, tmp_path, f["initial"], record_packings=True)
    checked = 0
    for e in range(2 * E):
        coach.rewards_list = [float(x) for x in f["ep_before"][e, :int(f["ep_before_len"][e])]]
        scores, _ = coach.selfPlayIteration(1 + e // E, draws=(int(f["ep_bin_height"][e]), [int(f["ep_seed"][e])]), move_rule=_lib.MOVE_ARGMAX_FIRST)
        (p,) = coach._selfplay.pop_packings()
        sel = np.nonzero(f["ex_ep"] == e)[0]
        assert p.moves == len(sel) and np.array_equal(p.item_wh, f["ep_items"][e])
        assert np.array_equal(p.board_after(-1), f["ex_rows"][sel[0]])
        for m in range(p.moves - 1):
            assert np.array_equal(p.board_after(m), f["ex_rows"][sel[m + 1]]), (e, m)
            checked += 1
        assert np.array_equal(p.board_after(p.moves - 1), p.board) and p.layout().shape == (int(f["H"]), int(f["W"]))
        assert p.score == float(f["ep_score"][e]) == scores[0] and p.outcome == int(f["ex_r"][sel[0]])
    assert checked > 2 * E
    coach._selfplay.close()


# ---- the engine's own golden-pinned rules as the referee (production path: no oracle search of the CNN's games) ------------------
def replay_with_engine_rules(eng, p, total_area, rewards, W, H, N):
    """The Packing's actions through rp_apply_move -> every move's rows and the final board must be the trace's; rp_game_ended on the
    final state -> outcome and score."""
    rows = np.zeros((1, H), np.uint64); rem = np.ones((1, N), np.uint8)
    wh = p.item_wh[None]
    for m in range(p.moves):
        nrows, rem, st = eng.apply_move(rows, rem, wh, [int(p.actions[m])])
        assert st[0] == 0
        changed = sum(1 << int(r) for r in np.flatnonzero(nrows[0] != rows[0]))
        assert changed == int(p.rows[m]), (p.episode_id, m)
        assert np.array_equal(p.board_after(m), nrows[0]), (p.episode_id, m)
        rows = nrows
    assert np.array_equal(rows[0], p.board)
    ended, r = eng.game_ended(rows, rem, wh, [total_area], [int(p.item_wh[:, 1].max())], rewards, ALPHA)
    assert ended[0] != 0 and r[0] == p.score
    if ended[0] != 2:  # 2: the r == bl tie, drawn by the salted rule
        assert ended[0] == p.outcome
    lay = p.layout()
    assert np.array_equal(ev.pack_board(lay >= 0), p.board)


def cnn_setup(W=10, H=10, N=8, sims=25, seed=0, **extra):
    import torch
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.binpacking.pytorch.NNet import NNetWrapper
    from resource_packing_self_play_amd.utils import dotdict
    args = dotdict(dict(numMCTSSims=sims, cpuct=1, alpha=ALPHA, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8), **extra)
    game = BinPackingGame(W, H, N, 1)
    torch.manual_seed(seed)
    return game, NNetWrapper(game, args), args


def test_production_path_records_every_packing():
    """CNN evaluator, HIP graphs, two groups, compact rows, auto-restart: three times more instances than slots."""
    import torch
    from resource_packing_self_play_amd import _lib
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    W, H, N, sims, games, n_inst = 10, 10, 8, 25, 16, 48
    game, nnet, args = cnn_setup(W, H, N, sims)
    rng = np.random.default_rng(8)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(n_inst)])
    area = np.full(n_inst, W * H, np.int32)
    buf = [0.8, 0.9, 1.0, 0.85]
    runs = []
    for on in (True, False):
        sp = BatchedSelfPlay(game, nnet, args, games=games, move_rule=_lib.MOVE_SAMPLE, seed=77, groups=2, max_examples=n_inst * N, use_graph=True,
                             compact_rows=True, tie_salt=3, record_packings=on)
        ids, outcome, score, moves, _ = sp.run(wh, area, buf, first_id=500)
        rep = sp.examples_packed()
        packs = sp.pop_packings()
        planes, pi, value = rep.dense()
        runs.append((ids, outcome, score, moves, rep.key.cpu().numpy(), rep.episode.cpu().numpy(), rep.move.cpu().numpy(), rep.wh.cpu().numpy(),
                     planes.cpu().numpy(), pi.cpu().numpy(), value.cpu().numpy()))
        if on:
            assert [p.episode_id for p in packs] == list(range(500, 500 + n_inst)) == list(ids)  # every episode exactly once
            assert sp.pop_packings() == []
            keys, ep, mv = runs[0][4], runs[0][5], runs[0][6]
            for k, p in enumerate(packs):
                assert np.array_equal(p.item_wh, wh[k]) and p.moves == moves[k] and p.score == score[k] and p.outcome == outcome[k]
                replay_with_engine_rules(sp.eng, p, W * H, buf, W, H, N)
                sel = np.flatnonzero(ep == p.episode_id)
                assert list(mv[sel]) == list(range(p.moves))
                for j in sel:  # the recorded state of example (episode, move) is the board before that move
                    assert np.array_equal(keys[j, :H].view(np.uint32).astype(np.uint64), p.board_after(int(mv[j]) - 1)), (k, int(mv[j]))
            print(packs[0])
        else:
            assert packs == []
            with pytest.raises(_lib.EngineError) as ei:
                sp.eng.pop_finished(packings=True)
            assert ei.value.code == _lib.ERR_ARG
        sp.close()
    for a, b in zip(*runs):  # the trace changes nothing it does not add
        assert np.array_equal(a, b)
    torch.cuda.synchronize()


def test_ring_chunks_switch_and_refusals():
    from resource_packing_self_play_amd import _lib
    W, H, N, sims, games = 10, 10, 8, 12, 13
    wh, buf = setup_games(W, H, N, games)
    eng = _lib.Engine(W, H, N, games, sims, alpha=ALPHA, move_rule=_lib.MOVE_ARGMAX_FIRST, seed=1, tie_salt=2)
    with pytest.raises(_lib.EngineError) as ei:  # trace off
        eng.pop_finished(packings=True)
    assert ei.value.code == _lib.ERR_ARG and "trace" in str(ei.value)
    eng.set_trace(True)
    eng.set_rank_buffer(buf)
    eng.begin_episodes(wh, np.full(games, W * H, np.int32), episode_id=np.arange(games) + 10)
    for on in (False, True):  # refused while episodes are being played, in either direction
        with pytest.raises(_lib.EngineError) as ei:
            eng.set_trace(on)
        assert ei.value.code == _lib.ERR_STATE
    run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: 2))
    # chunks smaller than the number finished, the plain pop in between: one ring, one cursor
    a = eng.pop_finished(max_n=5, packings=True)
    b = eng.pop_finished(max_n=3)
    c = eng.pop_finished(max_n=4, packings=True)
    d = eng.pop_finished(packings=True)
    e = eng.pop_finished(packings=True)
    assert [len(x[0]) for x in (a, b, c, d, e)] == [5, 3, 4, 1, 0]
    ids = np.concatenate([x[0] for x in (a, b, c, d)])
    assert sorted(int(i) for i in ids) == list(range(10, 10 + games))
    for part in (a, c, d):  # every record's trace belongs to ITS episode: it replays to its own final board with that episode's items
        for k, i in enumerate(part[0]):
            g = int(i) - 10
            m = int(part[3][k])
            masks, final = oracle_replay(W, H, N, wh[g], part[4][k, :m])
            assert np.array_equal(masks, part[5][k, :m]) and np.array_equal(final, part[6][k]) and not part[4][k, m:].any() and not part[5][k, m:].any()
    # a second set of episodes on the same context: shorter games leave no stale entries behind, the ring rewinds
    eng.begin_episodes(wh[::-1].copy(), np.full(games, W * H, np.int32), episode_id=np.arange(games) + 100)
    run_until_idle(eng, host_evaluator(lambda s: "hashed", W * N, lambda s: 2))
    got = records(eng)
    assert sorted(got) == list(range(100, 100 + games))
    for g in range(games):
        o, s, m, act, rows, board = got[100 + g]
        masks, final = oracle_replay(W, H, N, wh[games - 1 - g], act[:m])
        assert np.array_equal(masks, rows[:m]) and np.array_equal(final, board) and not act[m:].any() and not rows[m:].any()
    eng.set_trace(False)
    with pytest.raises(_lib.EngineError):
        eng.pop_finished(packings=True)
    eng.close()


def test_pack_returns_instance_order_and_repeats():
    from resource_packing_self_play_amd.binpacking.BinPackingGame import ItemsGenerator
    from resource_packing_self_play_amd.solve import pack
    W, H, N, sims = 10, 10, 8, 16
    game, nnet, args = cnn_setup(W, H, N, sims)
    rng = np.random.default_rng(3)
    wh = np.stack([gen_items(rng, W, H, N) for _ in range(20)])
    a = pack(game, nnet, args, item_wh=wh, games=8)  # more instances than slots: auto-restart, and more than one run of the driver
    assert [p.episode_id for p in a] == list(range(20)) and all(np.array_equal(p.item_wh, wh[k]) for k, p in enumerate(a))
    for p in a:
        assert np.array_equal(ev.pack_board(p.layout() >= 0), p.board) and 0.0 <= p.score <= 1.0
        assert p.score == 0.0 or p.score == max(int(np.ceil(W * H / W)), int(p.item_wh[:, 1].max())) / p.height  # BinPackingGame.py:193-198
    b = pack(game, nnet, args, item_wh=wh, games=8)  # greedy "lowest": nothing is drawn
    assert a == b
    seeds = [7, 3, 99, 12345, 3, 41]
    gen = ItemsGenerator(W, 8, N)
    state = np.random.get_state()
    want = np.array([[it[:2] for it in gen.items_generator(s)] for s in seeds], np.uint8)
    np.random.set_state(state)
    c = pack(game, nnet, args, seeds=seeds, bin_h=8, games=4)
    assert [p.episode_id for p in c] == list(range(6)) and all(np.array_equal(p.item_wh, want[k]) for k, p in enumerate(c))
    assert c[1].actions.tolist() == c[4].actions.tolist() and c[1].score == c[4].score  # the same seed twice
    assert c == pack(game, nnet, args, seeds=seeds, bin_h=8, games=4)


# ---- arena and gate -----------------------------------------------------------------------------------------------------------
def make_arena_coach(tmp, **over):
    from resource_packing_self_play_amd.CoachBPP import CoachBPP
    from resource_packing_self_play_amd.binpacking.BinPackingGame import ItemsGenerator
    W, H, N = 10, 10, 8
    kw = dict(numIters=2, numEps=8, iterStepThreshold=5, binH_min=7, binH=10, numScoresForRank=20, numItersForTrainExamplesHistory=5, maxlenOfQueue=200000,
              numItems=N, checkpoint=str(tmp), sample_seed=31337, arena_seed=5, arenaCompare=6, use_graph=True, groups=2, tie_salt=4)
    kw.update(over)
    game, nnet, args = cnn_setup(W, H, N, 16, seed=0, **kw)
    gen = ItemsGenerator(W, H, N)
    return CoachBPP(game, nnet, gen.items_generator(100), W * H, gen, args, saved_rewards_list=[0.7, 0.8, 0.9, 1.0]), game, args


def test_arena_playing(tmp_path):
    import torch
    from resource_packing_self_play_amd.MCTS_bpp import MCTS
    from resource_packing_self_play_amd.binpacking.pytorch.NNet import NNetWrapper
    from resource_packing_self_play_amd.solve import pack
    coach, game, args = make_arena_coach(tmp_path)
    seeds_iter = list(range(1000, 1040))
    assert coach.arena_playing(coach.nnet, coach.nnet, seeds_iter) == 1
    la = coach.last_arena
    assert np.array_equal(la["p_scores"], la["n_scores"]) and len(la["seeds"]) == 6 and set(la["seeds"]) <= set(seeds_iter) and la["accepted"] == 1
    first_seeds = list(la["seeds"])
    torch.manual_seed(1)
    other = NNetWrapper(game, args)
    before = {k: v.detach().clone() for k, v in coach.nnet.nnet.state_dict().items()}
    got = coach.arena_playing(MCTS(game, coach.nnet, args), MCTS(game, other, args), seeds_iter)
    la = coach.last_arena
    assert la["seeds"] == first_seeds  # args.arena_seed pins the draw
    for k, v in coach.nnet.nnet.state_dict().items():  # the driver's network got its own weights back, bit for bit
        assert torch.equal(v, before[k]), k
    coach._selfplay.close()
    # each network packing the same instances on its own, in a driver of the same shape.  The search reads the rank buffer and the
    # tie salt (a terminal's value is its outcome against the buffer, CoachBPP.py:259,265), so pack() gets the Coach's.
    same = dict(seeds=la["seeds"], bin_h=coach.gen.bin_height, rewards_list=coach.rewards_list, tie_salt=args.tie_salt, games=8, groups=2)
    want_p = [p.score for p in pack(game, coach.nnet, args, **same)]
    want_n = [p.score for p in pack(game, other, args, **same)]
    print("arena: old %s new %s" % (la["p_scores"].tolist(), la["n_scores"].tolist()))
    assert la["p_scores"].tolist() == want_p and la["n_scores"].tolist() == want_n
    assert got == la["accepted"] == (1 if np.mean(want_n) >= np.mean(want_p) else 0)


def run_gated_learn(tmp, verdict, **over):
    """learn() for two iterations with arena_playing patched to `verdict` (an int, or an exception to raise) -> (coach, per iteration:
    weights before training, weights after the iteration)."""
    coach, game, args = make_arena_coach(tmp, **over)
    calls, before, after = [], [], []
    state = lambda: {k: v.detach().clone() for k, v in coach.nnet.nnet.state_dict().items()}

    def arena(pmcts, nmcts, seeds_iter):
        calls.append(list(seeds_iter))
        if isinstance(verdict, Exception):
            raise verdict
        return verdict
    coach.arena_playing = arena
    train = coach.nnet.train_packed
    coach.nnet.train_packed = lambda rep: (before.append(state()), train(rep))[1]
    save = coach.save_rewards_list
    coach.save_rewards_list = lambda: (after.append(state()), save())[1]  # the last statement of an iteration
    coach.learn()
    coach._selfplay.close()
    return coach, game, args, calls, before, after


def test_gate_rejects(tmp_path):
    import torch
    coach, game, args, calls, before, after = run_gated_learn(tmp_path, 0, arena_gate=True)
    assert len(calls) == 2 and len(before) == 2 and len(after) == 2 and all(len(c) == 8 for c in calls)
    for it in range(2):
        for k in before[it]:
            assert torch.equal(before[it][k], after[it][k]), (it, k)  # load_checkpoint(temp.pth.tar)
    assert not os.path.exists(os.path.join(str(tmp_path), "best.pth.tar")) and os.path.exists(os.path.join(str(tmp_path), "temp.pth.tar"))
    assert [m["arena accepted"] for m in coach.metrics_log] == [0, 0] and all("arena_s" in t for t in coach.timings)


def test_gate_accepts(tmp_path):
    import torch
    from resource_packing_self_play_amd.binpacking.pytorch.NNet import NNetWrapper
    coach, game, args, calls, before, after = run_gated_learn(tmp_path, 1, arena_gate=True)
    assert len(calls) == 2
    for it in range(2):
        assert any(not torch.equal(before[it][k], after[it][k]) for k in before[it])
    torch.manual_seed(9)
    fresh = NNetWrapper(game, args)
    fresh.load_checkpoint(folder=str(tmp_path), filename="best.pth.tar")
    for k, v in fresh.nnet.state_dict().items():
        assert torch.equal(v, after[1][k]), k
    assert [m["arena accepted"] for m in coach.metrics_log] == [1, 1]


def test_no_arena_without_the_gate(tmp_path):
    coach, game, args, calls, before, after = run_gated_learn(tmp_path, RuntimeError("arena_playing called without args.arena_gate"))
    assert calls == [] and len(after) == 2 and coach.last_arena is None
    assert all("arena accepted" not in m for m in coach.metrics_log) and all("arena_s" not in t for t in coach.timings)
    assert not os.path.exists(os.path.join(str(tmp_path), "best.pth.tar"))


@pytest.mark.timeout(900)
def test_two_ranks_reach_the_same_arena_decision(tmp_path):
    """World size 2 (gloo, both ranks on this box's GPU; tests/dist_arena_worker.py): one unpatched gated iteration ends with the same
    accepted flag, the same arena score arrays and bit-identical weights on both ranks, and with the one-rank run's arena result."""
    outs = {}
    for world in (1, 2):
        procs = []
        port = 31500 + (os.getpid() % 2000) + world
        for r in range(world):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       RP_DIST_BACKEND="gloo", RP_SINGLE_DEVICE="1")
            procs.append(subprocess.Popen([sys.executable, "-X", "faulthandler", os.path.join(HERE, "dist_arena_worker.py"), str(tmp_path), str(world)], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        try:
            logs = [p.communicate(timeout=400)[0] for p in procs]
        finally:
            for p in procs:  # a rank that is still there after the limit (or after its peer failed) is ended; nothing follows a failure
                if p.poll() is None:
                    p.kill()
        assert all(p.returncode == 0 for p in procs), "world %d failed:\n%s" % (world, "\n".join("---- rank %d (rc %s)\n%s" % (r, p.returncode, o[-2500:]) for r, (p, o) in enumerate(zip(procs, logs))))
        for r in range(world):
            outs[(world, r)] = np.load(os.path.join(str(tmp_path), "arena_w%d_r%d.npz" % (world, r)))
    a, b, solo = outs[(2, 0)], outs[(2, 1)], outs[(1, 0)]
    wkeys = [k for k in a.files if k.startswith("w__")]
    assert len(wkeys) == 36
    for key in ["accepted", "seeds", "p_scores", "n_scores", "scores"] + wkeys:
        assert np.array_equal(a[key], b[key]), key
    print("two ranks: accepted %d, old %s, new %s; one rank: accepted %d, new %s" % (int(a["accepted"]), a["p_scores"].tolist(), a["n_scores"].tolist(),
                                                                                     int(solo["accepted"]), solo["n_scores"].tolist()))
    for key in ("accepted", "seeds", "p_scores", "n_scores", "scores"):
        assert np.array_equal(a[key], solo[key]), key
    assert len(a["seeds"]) == 5 and set(a["seeds"].tolist()) <= set(a["iter_seeds"].tolist())
