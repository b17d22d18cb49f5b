"""The incumbent of an episode with playouts as candidates (include/rp_engine.h: rp_set_incumbent_playouts) out of the CPU oracle.  Test
infrastructure.

The episode is searched by OracleMCTS with the restated playout evaluator (tests/rollout_ref.py), wrapped so that every evaluated state
is logged with the playouts it ran and the number of moves played at that time; it is played move by move with the loop of
tests/initial_ref.py (play_from), so the node count after every move's search is known as well.  OracleMCTS.dump() lists the nodes in
creation order, and the search creates one node per simulation: a terminal, or a leaf that is evaluated on the spot.  So the dump IS the
candidate sequence in simulation order.  A terminal makes one candidate as in best_ref.best_of_dump.  A non-terminal makes the offer
of its playouts: the largest score, the lowest playout index among equals.  A candidate replaces the incumbent iff there is none yet or
its score is strictly greater.  The evaluator's call log must equal the dump's non-terminal nodes in the same order: asserted here.
"""
import numpy as np

import best_ref
import evaluators as ev
import initial_ref as ir
import oracle_lib as orc
import rollout_ref as rr

ALPHA, BUF, SEED, SALT = best_ref.ALPHA, best_ref.BUF, best_ref.SEED, best_ref.SALT
ARGMAX_FIRST, SAMPLE = ir.ARGMAX_FIRST, ir.SAMPLE
PLAYOUTS = 3  # of the probe over best_ref.SHAPES


class _Cut(Exception):
    pass


def episode(W, H, N, wh, area, buf, sims, policy, seed, salt, eid, playouts, board=None, rem=None, max_moves=None):
    """One episode of the oracle from (board [H, W] cells, rem [N]; default: the empty bin, all items) -> dict:
      played: dict of initial_ref.play_from (actions, outcome, score, moves, board)
      sizes: uint8 [N, 2] the sizes the oracle played with (absent items 0)
      bounds: node count after the search of every move; history: one record per update of the incumbent, in order
      score, outcome, rows, rem, moves, prefix, tree_moves, playout, actions, leaf, updates, node, tied: the last of them (the incumbent)
      sources: the `playout` of every update ("-1" = a tree terminal); tied_wins: winning offers whose maximum several playouts share
      tree: best_ref.best_of_dump of the same tree (the tree-only incumbent), None for an episode of 0 moves
    max_moves: stop behind the search of that many moves (no move is played after it): `played` is None and `tree` is not computed.
    A record: score, outcome, rows uint64 [H], rem uint8 [N], moves, prefix (moves played when it was found), tree_moves (actions to the
    leaf, == moves for a terminal), playout (index or -1), actions (the playout's own action list, None for a terminal), leaf ((rows,
    rem) of the evaluated state, None for a terminal), updates (its number, from 1), node (index in creation order), tied."""
    board = np.zeros((H, W), np.uint8) if board is None else np.array(board, np.uint8).reshape(H, W)
    rem = np.ones(N, np.uint8) if rem is None else (np.asarray(rem) != 0).astype(np.uint8)
    start = int(rem.sum())
    sizes = (np.asarray(wh, np.uint8) * rem[:, None]).astype(np.uint8)
    max_h = ir.default_max_h(wh, rem)
    plain = rr.evaluator(W, H, N, sizes, area, buf, seed, salt, eid, playouts)
    log, state = [], dict(prefix=0, checked=False)

    def logged(b, r):
        runs = [rr.playout(W, H, N, b, r, sizes, area, buf, seed, salt, eid, j) for j in range(playouts)]
        pi = np.full(W * N, np.float32(1) / np.float32(W * N), dtype=np.float32)
        v = np.array([np.float32(sum(x[0] for x in runs)) / np.float32(playouts)], dtype=np.float32)
        if not state["checked"]:  # the wrapper returns what rollout_ref.evaluator returns
            p0, v0 = plain(b, r)
            assert np.array_equal(p0, pi) and np.array_equal(v0, v)
            state["checked"] = True
        log.append(dict(rows=ev.pack_board(b).copy(), rem=np.array(r, np.uint8), prefix=state["prefix"], runs=runs))
        return pi, v

    m = orc.OracleMCTS(W, H, N, 1.0, ALPHA, logged, lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))
    ir.begin(m, wh, rem, area, buf, salt)
    assert m.episode["max_h"] == max_h
    bounds, search = [], m.action_counts

    def counted(b, r, n):  # play_from searches once per move
        state["prefix"] = len(bounds)
        counts = search(b, r, n)
        bounds.append(int(orc.lib().orc_mcts_num_nodes(m.h)))
        if max_moves is not None and len(bounds) == max_moves:
            raise _Cut()
        return counts

    m.action_counts = counted
    try:
        played = ir.play_from(m, board, rem, sims, policy, seed, eid)
    except _Cut:
        played = None
    dump = m.dump()
    m.close()
    out = dict(played=played, sizes=sizes, bounds=bounds, history=[], sources=[], tied_wins=0, tree=None)
    if played is not None and not played["moves"]:
        return out
    if played is not None:
        out["tree"] = best_ref.best_of_dump(dump, W, H, area, max_h, buf)
    best, evaluated = None, 0
    for node, ((rows_b, rem_b), rec) in enumerate(dump.items()):
        rows, nrem = np.frombuffer(rows_b, np.uint64), np.frombuffer(rem_b, np.uint8)
        prefix = next(k for k, bound in enumerate(bounds) if node < bound)
        if rec["es"] != 0:
            _, r = orc.ranked_reward(W, H, ev.unpack_board(rows, W), area, max_h, buf, ALPHA)
            moves = start - int(nrem.sum())
            cand = dict(score=r, outcome=int(rec["es"]), rows=rows.copy(), rem=nrem.copy(), moves=moves, prefix=prefix, tree_moves=moves, playout=-1,
                        actions=None, leaf=None, tied=False)
        else:
            call = log[evaluated]
            assert np.array_equal(call["rows"], rows) and np.array_equal(call["rem"], nrem), "evaluation %d is not node %d" % (evaluated, node)
            assert call["prefix"] == prefix
            evaluated += 1
            scores = [x[1] for x in call["runs"]]
            top = max(scores)
            j = scores.index(top)  # the lowest index among the maxima
            e, r, pm, final = call["runs"][j]
            tree_moves = start - int(nrem.sum())
            cand = dict(score=r, outcome=e, rows=np.array(final, np.uint64), rem=None, moves=tree_moves + pm, prefix=prefix, tree_moves=tree_moves,
                        playout=j, actions=None, leaf=(rows.copy(), nrem.copy()), tied=scores.count(top) > 1)
        if best is None or cand["score"] > best["score"]:
            if cand["playout"] >= 0:  # the winner's own moves: the same playout once more, traced
                trace = []
                _, fb, fr = rr.playout_path(W, H, N, ev.unpack_board(rows, W), nrem, sizes, seed, eid, cand["playout"], trace=trace)
                assert np.array_equal(ev.pack_board(fb), cand["rows"]) and len(trace) == cand["moves"] - cand["tree_moves"]
                cand.update(rem=np.array(fr, np.uint8), actions=[t[3] for t in trace])
            best = dict(cand, updates=len(out["history"]) + 1, node=node)
            out["history"].append(best)
            out["sources"].append(best["playout"])
            out["tied_wins"] += bool(best["tied"])
    assert evaluated == len(log), "the evaluator was called for a state that is not in the tree"
    out.update(best)
    return out


def running(ref, moves_played):
    """The incumbent once the search of move number `moves_played` (from 0) is complete: the last update among the nodes created so far;
    None if there is none yet."""
    seen = [h for h in ref["history"] if h["node"] < ref["bounds"][moves_played]]
    return seen[-1] if seen else None


def probe(shape, g, playouts=PLAYOUTS, policy=SAMPLE):
    """Episode g of best_ref.SHAPES[shape] as the probe plays it: best_ref.BUF, seed 5, salt 9, episode id g -> (wh [N, 2], episode())."""
    W, H, bin_h, N, sims, games = best_ref.SHAPES[shape]
    wh = best_ref.instances(W, bin_h, N, games)[g]
    return wh, episode(W, H, N, wh, W * bin_h, BUF, sims, policy, SEED, SALT, g, playouts)


# ---- late-game starts: a tree terminal replaces a playout incumbent -------------------------------------------------------------------------
# 10x10 board, engine N = 8, only item 0 = (2, 3) takes part, every column filled from row 0 to a height drawn per instance; one playout,
# 12 simulations, the first argmax.  The root's playout is the first candidate (P); the tree then tries every column, and where one of
# them scores strictly higher the record ends as a tree terminal (T).
LATE_W, LATE_H, LATE_N, LATE_SIMS, LATE_PLAYOUTS, LATE_COUNT = 10, 10, 8, 12, 1, 12
LATE_P_THEN_T = (0, 2, 5, 7, 9, 11)  # the instances whose updates are P then T (test_best_playout_cpu.py checks the list)


def late_instances():
    """-> (wh uint8 [12, N, 2] as the engine takes them (absent items 1x1), boards uint8 [12, H, W], rem uint8 [12, N], areas int32 [12])."""
    rng = np.random.default_rng(7)
    wh = np.ones((LATE_COUNT, LATE_N, 2), np.uint8)
    wh[:, 0] = (2, 3)
    rem = np.zeros((LATE_COUNT, LATE_N), np.uint8)
    rem[:, 0] = 1
    boards = np.zeros((LATE_COUNT, LATE_H, LATE_W), np.uint8)
    for k in range(LATE_COUNT):
        heights = rng.integers(0, 6, LATE_W)
        for c in range(LATE_W):
            boards[k, :int(heights[c]), c] = 1
    areas = (boards.reshape(LATE_COUNT, -1).sum(axis=1) + 6).astype(np.int32)  # the default: the set cells plus the items that take part
    return wh, boards, rem, areas


def late_episode(k, inst=None):
    wh, boards, rem, areas = inst or late_instances()
    return episode(LATE_W, LATE_H, LATE_N, wh[k], int(areas[k]), BUF, LATE_SIMS, ARGMAX_FIRST, SEED, SALT, k, LATE_PLAYOUTS, boards[k], rem[k])
