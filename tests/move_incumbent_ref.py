"""An episode under RP_MOVE_INCUMBENT (include/rp_engine.h: rp_move_rule) restated over the CPU oracle.  Test infrastructure.

The oracle does not keep the path that created a node, and the rule plays along the incumbent's ACTION LIST.  So the episode is searched
one simulation at a time -- OracleMCTS.action_counts(board, rem, 1), the loop of orc_mcts_action_counts with n_sims, which leaves the
same tree -- and after every simulation its path is read off the tree: the chain of edges from the current root whose nsa grew.  A
simulation changes nsa on its own path only and passes through a state at most once (every move places an item), so a cache of the visit
counts of every state a path has touched says which edge grew; the chain ends where none did.  Where the simulation created a node the
chain ends at that node: asserted.

The candidates of the incumbent, in simulation order, are those of best_ref (a new terminal node) and, with playouts, of
best_playout_ref (a new leaf's best playout: the largest score, the lowest index among equals); a terminal that a played move
materialises -- the rule may play a move the search never tried -- is one too, behind the move's simulations.  A candidate replaces the
incumbent iff there is none yet or its score is strictly greater.  Since the path is known, so is every incumbent's action list: the
GPU tests compare lists for equality.

The move: the incumbent I is followable iff it exists, I.score > 0, I.moves > the moves played and I.actions[:moves played] == the
played actions; then the move is I.actions[moves played], else the first argmax of the root's visit counts.  switch_at = k: moves below
k are the first argmax whatever the incumbent says (RP_MOVE_ARGMAX_FIRST, then rp_set_move_rule(4) before move k).
"""
import ctypes as C

import numpy as np

import best_ref
import evaluators as ev
import oracle_lib as orc
import playout_landing_ref as pl
import rollout_ref as rr

ALPHA, BUF, SEED, SALT = best_ref.ALPHA, best_ref.BUF, best_ref.SEED, best_ref.SALT
NEVER = 1 << 30  # switch_at of an episode played by RP_MOVE_ARGMAX_FIRST throughout
UNIFORM, WIDTH2 = (0, 0), (2, 0)  # playout policies (w_pow, h_pow)
FIELDS = ("score", "outcome", "rows", "moves", "prefix", "updates", "actions", "tree_moves", "playout")


def _node(m, i):
    """Node i of the oracle in creation order -> (board cells [H, W], rem [N], es)."""
    W, H, N, A = m.W, m.H, m.N, m.A
    board = np.zeros(H * W, np.uint8); rem = np.zeros(N, np.uint8)
    valids = np.zeros(A, np.uint8); p = np.zeros(A, np.float64); nsa = np.zeros(A, np.uint32); q = np.zeros(A, np.float64); qk = np.zeros(A, np.uint8)
    es, esk, exp, ns = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
    u8 = C.POINTER(C.c_uint8)
    orc.lib().orc_mcts_get_node(m.h, i, board.ctypes.data_as(u8), rem.ctypes.data_as(u8), C.byref(es), C.byref(esk), C.byref(exp), C.byref(ns),
                                valids.ctypes.data_as(u8), p.ctypes.data_as(C.POINTER(C.c_double)), nsa.ctypes.data_as(C.POINTER(C.c_uint32)),
                                q.ctypes.data_as(C.POINTER(C.c_double)), qk.ctypes.data_as(u8))
    return board.reshape(H, W), rem, int(es.value)


def _key(board, rem):
    return board.tobytes(), (np.asarray(rem) != 0).astype(np.uint8).tobytes()


def episode(W, H, N, wh, area, buf, sims, eid, kind=None, playouts=0, policy=UNIFORM, land_pow=0, seed=SEED, salt=SALT, switch_at=0,
            want_tree=False):
    """One episode from the empty bin with all items.  kind: a table evaluator of tests/evaluators.py (tree terminals are the only
    candidates); or playouts > 0: the rollout restatement under (policy, land_pow), each new leaf's best playout a candidate too.
    -> dict:
      actions, outcome, score, board (uint64 [H], the final bin): the played episode
      followed: per move, whether it followed the incumbent; fallback_counts: per move the root's visit counts uint32 [A]
      running: per move the incumbent once the move's search is complete (None: none yet); a record has FIELDS -- rows uint64 [H],
        actions the whole list from the initial state, tree_moves == moves and playout == -1 for a tree terminal
      history: every update in order, each with `at` = the moves played when it was found; best: the last one
      off_line: the moves at which the incumbent scored above 0 and had a next action but its line did not pass through the root
      tree: OracleMCTS.dump() of the final tree (want_tree)"""
    wh = np.asarray(wh, np.uint8)
    iw, ih = wh[:, 0], wh[:, 1]
    max_h, A = int(ih.max()), W * N
    uniform = policy == UNIFORM and land_pow == 0
    log = []

    def run(b, r, j):
        if uniform:
            return rr.playout(W, H, N, b, r, wh, area, buf, seed, salt, eid, j)
        return pl.playout(W, H, N, b, r, wh, area, buf, seed, salt, eid, j, policy=policy, land_pow=land_pow)

    def rollout_eval(b, r):
        runs = [run(b, r, j) for j in range(playouts)]
        log.append(runs)
        return (np.full(A, np.float32(1) / np.float32(A), dtype=np.float32),
                np.array([np.float32(sum(x[0] for x in runs)) / np.float32(playouts)], dtype=np.float32))

    table_eval = lambda b, r: ev.table_eval(kind, ev.pack_board(b), r, A, salt)
    m = orc.OracleMCTS(W, H, N, 1.0, ALPHA, rollout_eval if playouts else table_eval, lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))
    m.begin_episode(iw, ih, area, buf)
    cache, known, zeros = {}, set(), np.zeros(A, np.uint32)
    out = dict(actions=[], followed=[], fallback_counts=[], running=[], history=[], off_line=[], best=None)
    state = dict(inc=None)

    def offer(cand):
        inc = state["inc"]
        if inc is None or cand["score"] > inc["score"]:
            cand = dict(cand, updates=len(out["history"]) + 1, at=len(out["actions"]))
            assert cand["moves"] == len(cand["actions"])
            state["inc"] = cand
            out["history"].append(cand)

    def terminal(b, r, es, actions, prefix):
        _, score = orc.ranked_reward(W, H, b, area, max_h, buf, ALPHA)
        return dict(score=float(score), outcome=es, rows=ev.pack_board(b).copy(), moves=len(actions), prefix=prefix, actions=list(actions),
                    tree_moves=len(actions), playout=-1)

    def walk(b, r):
        """The latest simulation's path from (b, r) -> (actions, end board, end rem); brings the cache up to date along it."""
        path = []
        while True:
            k = _key(b, r)
            now, before = m.action_counts(b, r, 0), cache.get(k, zeros)
            grown = np.flatnonzero(now != before)
            cache[k] = now
            if not len(grown):
                return path, b, r
            assert len(grown) == 1 and int(now[grown[0]]) == int(before[grown[0]]) + 1
            path.append(int(grown[0]))
            rc, b, r = orc.next_state(W, H, N, b, iw, ih, r, path[-1])
            assert rc == 0

    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    outcome = score = None
    while outcome is None:
        played = out["actions"]
        for _ in range(sims):
            n0, evals0 = int(orc.lib().orc_mcts_num_nodes(m.h)), len(log)
            m.action_counts(board, rem, 1)
            path, eb, er = walk(board, rem)
            n1 = int(orc.lib().orc_mcts_num_nodes(m.h))
            if n1 == n0:
                assert len(log) == evals0
                continue
            nb, nr, es = _node(m, n0)
            assert n1 == n0 + 1 and np.array_equal(nb, eb) and np.array_equal(nr != 0, er != 0), "the chain of grown edges does not end at the new node"
            known.add(_key(nb, nr))
            line = played + path
            if es != 0:
                assert len(log) == evals0
                offer(terminal(nb, nr, es, line, len(played)))
            elif playouts:
                assert len(log) == evals0 + 1
                scores = [x[1] for x in log[-1]]
                j = scores.index(max(scores))  # the lowest index among the maxima
                e, r, pm, final = log[-1][j]
                inc = state["inc"]
                if inc is None or r > inc["score"]:  # the winner's own moves: the same playout once more, traced
                    trace = []
                    if uniform:
                        rr.playout_path(W, H, N, nb, nr, wh, seed, eid, j, trace=trace)
                    else:
                        pl.playout_path(W, H, N, nb, nr, wh, seed, eid, j, trace=trace, policy=policy, land_pow=land_pow)
                    tail = [int(t[3]) for t in trace]
                    assert len(tail) == pm
                    offer(dict(score=float(r), outcome=int(e), rows=np.array(final, np.uint64), moves=len(line) + pm, prefix=len(played),
                               actions=line + tail, tree_moves=len(line), playout=j))
        # ---- the move -------------------------------------------------------------------------------------------------------------------
        inc, mv = state["inc"], len(played)
        out["running"].append(None if inc is None else dict(inc))
        counts = m.action_counts(board, rem, 0)
        out["fallback_counts"].append(counts)
        live = inc is not None and inc["score"] > 0 and inc["moves"] > mv
        on_line = live and inc["actions"][:mv] == played
        if live and not on_line:
            out["off_line"].append(mv)
        follow = bool(on_line) and mv >= switch_at
        if follow:
            action = int(inc["actions"][mv])
        else:
            action = int(np.argmax(counts))  # lowest index among the maxima
            assert counts[action] > 0
        out["followed"].append(follow)
        rc, board, rem = orc.next_state(W, H, N, board, iw, ih, rem, action)
        assert rc == 0, "the incumbent's next action is not legal at the root"
        is_end = not orc.has_valid_moves(W, H, N, board, iw, ih, rem)
        if is_end and _key(board, rem) not in known:  # a move the search never tried ended on a terminal nobody had seen: it is materialised
            n0 = int(orc.lib().orc_mcts_num_nodes(m.h))
            m.action_counts(board, rem, 1)
            nb, nr, es = _node(m, n0)
            assert int(orc.lib().orc_mcts_num_nodes(m.h)) == n0 + 1 and es != 0 and np.array_equal(nb, board)
            known.add(_key(nb, nr))
            offer(terminal(nb, nr, es, played + [action], mv))
        played.append(action)
        if is_end:
            e, score = orc.ranked_reward(W, H, board, area, max_h, buf, ALPHA)
            outcome = ev.tie_value(ev.pack_board(board), rem, salt) if e == rr.TIE else int(e)
    out.update(outcome=int(outcome), score=float(score), board=ev.pack_board(board), best=state["inc"], n_followed=sum(out["followed"]))
    if want_tree:
        out["tree"] = m.dump()
    m.close()
    return out


def check_invariant(ref):
    """Under the rule from the start of an episode: best.score > 0 -> the incumbent is the played packing."""
    best = ref["best"]
    assert best is not None and best["score"] >= ref["score"]
    if best["score"] > 0:
        assert best["actions"] == ref["actions"] and best["score"] == ref["score"] and best["outcome"] == ref["outcome"]
        assert np.array_equal(best["rows"], ref["board"])
    else:
        assert not any(ref["followed"])


def probe(shape, g, **kw):
    """Episode g of best_ref.SHAPES[shape] with the probe's settings: best_ref.BUF, salt 9, episode id g, evaluator KINDS[g % 2] unless
    playouts are asked for -> (wh [N, 2], episode())."""
    W, H, bin_h, N, sims, games = best_ref.SHAPES[shape]
    wh = best_ref.instances(W, bin_h, N, games)[g]
    if not kw.get("playouts"):
        kw.setdefault("kind", best_ref.KINDS[g % 2])
    return wh, episode(W, H, N, wh, W * bin_h, BUF, sims, g, **kw)


# ---- N > 64: the second lane pair of the prefix comparison -------------------------------------------------------------------------------------
BIG_W, BIG_H, BIG_N, BIG_SIMS, BIG_AREA = 12, 12, 70, 8, 72


def big_instance():
    """12x12 board, 70 items cut from 12x6: an episode of 70 moves."""
    return rr.cut_items(np.random.default_rng(3), BIG_W, 6, BIG_N)


def big_episode(kind, **kw):
    return episode(BIG_W, BIG_H, BIG_N, big_instance(), BIG_AREA, BUF, BIG_SIMS, 0, kind=kind, **kw)
