"""Python restatement of the playout policy (include/rp_engine.h: rp_set_playout_policy) over the oracle's rules.  Test infrastructure:
integer arithmetic and the oracle's C functions only, so the HIP kernels can be held to it bit for bit.  It parallels
rollout_ref.playout_path / playout / evaluator with one more argument, the policy (w_pow, h_pow); everything that does not change --
the stream, the ranking, the tie rule -- is rollout_ref's.

The sampling rule, as the header states it:
  - At step s of playout j, m_i is the legal-column mask of item i and c_i = popcount(m_i).
  - nv = sum c_i == 0 ends the playout.
  - Otherwise T = sum c_i * wt_i, wt_i = w_i^w_pow * h_i^h_pow.
  - pick = umulhi(sample(h0, j, s), T), the same stream: h0 = mix64(key_hash(S, seed) ^ e).
  - The legal moves lie in ascending action order (a = item * W + column).  Each move occupies wt_i consecutive units of [0, T).
    The move that owns unit `pick` is played:
      item   = the first i whose inclusive sum sum_{k<=i} c_k wt_k exceeds pick;
      column = set bit number floor((pick - sum_{k<i} c_k wt_k) / wt_i) of m_i, counted from 0.
  - Limits: w_pow >= 0, h_pow >= 0, w_pow + h_pow <= 2.  Then 1 <= wt_i <= 4096 and T <= 64 * 128 * 4096 = 2^25.
  - With (0, 0) the rule is the uniform one, bit for bit.
"""
import numpy as np

import evaluators as ev
import oracle_lib as orc
import rollout_ref as rr

UNIFORM = (0, 0)
NAMES = {"uniform": (0, 0), "area": (1, 1), "width": (1, 0), "width2": (2, 0), "height": (0, 1), "height2": (0, 2)}


def weights(wh, policy):
    """wt_i of every item -> list of Python ints."""
    w_pow, h_pow = policy
    assert w_pow >= 0 and h_pow >= 0 and w_pow + h_pow <= 2
    return [int(w) ** w_pow * int(h) ** h_pow for w, h in np.asarray(wh).reshape(-1, 2)]


def pick_move(mask, W, N, wt, x):
    """The move that draw x chooses among the legal moves of `mask` (uint8 [N * W]) -> (action, dict of the step: T, pick, item, bit =
    the column's number among the item's legal columns, c = legal columns of the item, wt = its weight, last = the pick fell in the
    last item that has a legal move)."""
    mask = np.asarray(mask).reshape(N, W)
    c = [int(k) for k in (mask != 0).sum(axis=1)]
    T = sum(c[i] * wt[i] for i in range(N))
    pick = rr.umulhi(x, T)
    before = 0
    for i in range(N):
        if before + c[i] * wt[i] > pick:
            break
        before += c[i] * wt[i]
    bit = (pick - before) // wt[i]
    last = max(k for k in range(N) if c[k])
    return i * W + int(np.flatnonzero(mask[i])[bit]), dict(T=T, pick=pick, item=i, bit=bit, c=c[i], wt=wt[i], last=i == last)


def playout_path(W, H, N, board, rem, wh, seed, episode_id, j, trace=None, policy=UNIFORM):
    """Plays playout j from (board [H, W] cells, rem [N]) under `policy` -> (moves, final board, final rem).  trace: a list that receives
    (legal-move mask, nv, draw x, action, step dict of pick_move) of every step -- rollout_ref's four fields, then the weighted ones."""
    board = np.array(board, np.uint8).reshape(H, W).copy(); rem = np.array(rem, np.uint8).copy()
    iw, ih = wh[:, 0], wh[:, 1]
    wt = weights(wh, policy)
    h0 = ev.splitmix64(ev.key_hash(ev.pack_board(board), rem, seed) ^ (int(episode_id) & ev.M64))
    moves = 0
    for s in range(N):  # every move places one item
        mask, nv = orc.valid_moves(W, H, N, board, iw, ih, rem)
        if nv == 0:
            break
        x = orc.lib().orc_sample_u64(h0, int(j), s)
        a, step = pick_move(mask, W, N, wt, x)
        if trace is not None:
            trace.append((mask, int(nv), int(x), a, step))
        rc, board, rem = orc.next_state(W, H, N, board, iw, ih, rem, a)
        assert rc == 0
        moves += 1
    return moves, board, rem


def playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j, policy=UNIFORM):
    """-> (outcome, score, moves, final rows uint64 [H])."""
    moves, fb, fr = playout_path(W, H, N, board, rem, wh, seed, episode_id, j, policy=policy)
    e, r = rr.rank(W, H, fb, fr, area, int(wh[:, 1].max()), buf, tie_salt)
    return e, r, moves, ev.pack_board(fb)


def evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=UNIFORM):
    """Closure with OracleMCTS's eval_py signature: (board, rem) -> (pi float32 [A], v float32 [1])."""
    A = W * N
    pi = np.full(A, np.float32(1) / np.float32(A), dtype=np.float32)

    def eval_py(board, rem):
        total = sum(playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j, policy=policy)[0] for j in range(playouts))
        return pi, np.array([np.float32(total) / np.float32(playouts)], dtype=np.float32)
    return eval_py


def oracle(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=UNIFORM):
    """OracleMCTS of one instance whose evaluator is the weighted restatement; begin_episode done."""
    m = orc.OracleMCTS(W, H, N, 1.0, rr.ALPHA, evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy),
                       lambda b, r: ev.tie_value(ev.pack_board(b), r, tie_salt))
    m.begin_episode(wh[:, 0], wh[:, 1], area, buf)
    return m


def under(monkeypatch, policy):
    """For the duration of a test, rollout_ref's playout functions are the weighted ones under `policy`: best_playout_ref.episode calls
    them by name, and with this it computes the incumbent of a search whose playouts follow the policy."""
    import functools
    for name in ("playout_path", "playout", "evaluator", "oracle"):
        monkeypatch.setattr(rr, name, functools.partial(globals()[name], policy=policy))


# ---- the states of the GPU parity test: shared with the CPU test that proves their coverage -------------------------------------------------
GPU_SEED, GPU_SALT = 20251, 77  # as tests/test_gpu_rollout.py plays the rollout_ref.GEOMETRIES cases
GPU_POLICIES = ((1, 1), (2, 0), (0, 2))
GPU_PLAYOUTS = 4


def random_state(rng, W, H, N, wh, n_moves):
    """The state n_moves uniformly drawn legal moves into the instance (fewer when it ends earlier)."""
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    for _ in range(n_moves):
        mask, nv = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        if nv == 0:
            break
        _, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, int(rng.choice(np.flatnonzero(mask))))
    return board, rem


def near_terminal_state(rng, W, H, N, wh):
    """Uniformly drawn moves until the state before the one without a legal move: at least one move is left, few are."""
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    while True:
        mask, nv = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        assert nv > 0
        _, nb, nr = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, int(rng.choice(np.flatnonzero(mask))))
        if orc.valid_moves(W, H, N, nb, wh[:, 0], wh[:, 1], nr)[1] == 0:
            return board, rem
        board, rem = nb, nr


def gpu_states(name):
    """The three states of geometry `name`: the start, a mid-game state and a near-terminal one, each of its own instance and with a
    non-zero episode id -> list of (item sizes, area, board, rem, episode id)."""
    W, H, N, _ = rr.GEOMETRIES[name]
    rng = np.random.default_rng(N * 23 + H)
    out = []
    for k in range(3):
        wh, area = rr.make_items(name, rng)
        if k == 0:
            board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
        elif k == 1:
            board, rem = random_state(rng, W, H, N, wh, max(2, N // 4))
        else:
            board, rem = near_terminal_state(rng, W, H, N, wh)
        out.append((wh, area, board, rem, 1000 * (k + 1) + 7))
    return out


def gpu_buffers(name):
    """The three buffers on the smallest geometry, one elsewhere."""
    return rr.BUFFERS if name == "10x10/8" else {"mixed": rr.BUFFERS["mixed"]}
