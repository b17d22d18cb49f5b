"""Python restatement of the random-playout leaf evaluator (include/rp_engine.h: rp_rollout_eval / rp_rollout_states) over the
oracle's rules.  Test infrastructure: integer arithmetic and the oracle's C functions only, so the HIP kernels can be held to it bit
for bit.

Playout j from state S of the episode with id e: h0 = splitmix64(key_hash(S, seed) ^ e); at step s the legal moves are counted (nv);
nv == 0 ends the playout, otherwise legal move number umulhi(orc_sample_u64(h0, j, s), nv) in ascending action order is played.  The
outcome is the ranked reward of the final bin, the r == bl tie drawn by evaluators.tie_value(final state, tie_salt); the leaf's value
is float32(sum of outcomes) / float32(K) and the prior is float32(1) / float32(A) everywhere.
"""
import numpy as np

import evaluators as ev
import oracle_lib as orc

TIE = 2  # orc_ranked_reward's sentinel of the r == bl branch

# the smallest geometries that reach every instantiation of the kernels: (W, H, N, kind of items)
GEOMETRIES = {
    "10x10/8": (10, 10, 8, "cut"),      # baseline
    "20x20/32": (20, 20, 32, "cut"),    # the c3 shape
    "40x6/12": (40, 6, 12, "cut"),      # 64-bit rows
    "12x12/70": (12, 12, 70, "small"),  # N > 64: the second remaining word; items of 1..3 cells per side overfill the bin -> dead ends
    "64x64/128": (64, 64, 128, "cut"),  # the ABI's limits
}
BUFFERS = {"empty": [], "zeros": [0.0, 0.0, 0.0, 0.0], "mixed": [0.5, 0.6, 0.7, 0.8]}
ALPHA = 0.75


def cut_items(rng, W, H, N):
    """Guillotine split of the W x H rectangle into N items, like ItemsGenerator (BinPackingGame.py:257-285) -> uint8 [N, 2] (w, h)."""
    items = [(W, H)]
    while len(items) < N:
        k = int(rng.integers(len(items))); w, h = items[k]
        if rng.integers(2) == 0:
            if w == 1:
                continue
            c = int(rng.integers(1, w)); items.pop(k); items += [(c, h), (w - c, h)]
        else:
            if h == 1:
                continue
            c = int(rng.integers(1, h)); items.pop(k); items += [(w, c), (w, h - c)]
    return np.array(items, np.uint8)


def make_items(name, rng):
    """Item sizes uint8 [N, 2] and the total area of one instance of GEOMETRIES[name]."""
    W, H, N, kind = GEOMETRIES[name]
    wh = cut_items(rng, W, H, N) if kind == "cut" else rng.integers(1, 4, size=(N, 2)).astype(np.uint8)
    return wh, int((wh[:, 0].astype(np.int64) * wh[:, 1]).sum())


def umulhi(x, n):
    return (int(x) * int(n)) >> 64


def playout_path(W, H, N, board, rem, wh, seed, episode_id, j, trace=None):
    """Plays playout j from (board [H, W] cells, rem [N]) -> (moves, final board, final rem).  trace: a list that receives
    (legal-move mask, nv, draw x, action) of every step."""
    board = np.array(board, np.uint8).reshape(H, W).copy(); rem = np.array(rem, np.uint8).copy()
    iw, ih = wh[:, 0], wh[:, 1]
    h0 = ev.splitmix64(ev.key_hash(ev.pack_board(board), rem, seed) ^ (int(episode_id) & ev.M64))
    moves = 0
    for s in range(N):  # every move places one item
        mask, nv = orc.valid_moves(W, H, N, board, iw, ih, rem)
        if nv == 0:
            break
        x = orc.lib().orc_sample_u64(h0, int(j), s)
        a = int(np.flatnonzero(mask)[umulhi(x, nv)])
        if trace is not None:
            trace.append((mask, int(nv), int(x), a))
        rc, board, rem = orc.next_state(W, H, N, board, iw, ih, rem, a)
        assert rc == 0
        moves += 1
    return moves, board, rem


def rank(W, H, board, rem, area, max_h, buf, tie_salt):
    """(outcome +-1, score r) of a final bin: the ranked reward with the tie drawn from the state."""
    e, r = orc.ranked_reward(W, H, board, area, max_h, buf, ALPHA)
    if e == TIE:
        e = ev.tie_value(ev.pack_board(board), rem, tie_salt)
    return int(e), float(r)


def playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j):
    """-> (outcome, score, moves, final rows uint64 [H])."""
    moves, fb, fr = playout_path(W, H, N, board, rem, wh, seed, episode_id, j)
    e, r = rank(W, H, fb, fr, area, int(wh[:, 1].max()), buf, tie_salt)
    return e, r, moves, ev.pack_board(fb)


def evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts):
    """Closure with OracleMCTS's eval_py signature: (board, rem) -> (pi float32 [A], v float32 [1])."""
    A = W * N
    pi = np.full(A, np.float32(1) / np.float32(A), dtype=np.float32)

    def eval_py(board, rem):
        total = sum(playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j)[0] for j in range(playouts))
        return pi, np.array([np.float32(total) / np.float32(playouts)], dtype=np.float32)
    return eval_py


def oracle(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts):
    """OracleMCTS of one instance whose evaluator is the restatement; begin_episode done."""
    m = orc.OracleMCTS(W, H, N, 1.0, ALPHA, evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts),
                       lambda b, r: ev.tie_value(ev.pack_board(b), r, tie_salt))
    m.begin_episode(wh[:, 0], wh[:, 1], area, buf)
    return m
