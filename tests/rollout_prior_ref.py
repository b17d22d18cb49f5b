"""Python restatement of the rollout prior (include/rp_engine.h: rp_set_rollout_prior) over the oracle's rules.  Test infrastructure:
integer arithmetic and the oracle's C functions only, so the HIP kernel can be held to it bit for bit.  It parallels
playout_policy_ref.evaluator / oracle with one more argument, the prior (w_pow, h_pow, land_pow); the playouts are playout_policy_ref's.

The rule, as the header states it:
  - For a leaf state, m_i is the legal-column mask of item i (getValidMoves, BinPackingGame.py:78-92).
  - A legal move (i, c) gets the integer weight u(i, c) = w_i^w_pow * h_i^h_pow * (H - t(i, c))^land_pow.
  - t(i, c) is the first row r, counted from 0, whose window [c, c + w_i) is empty: the t of get_adjacency
    (BinPackingLogic.py:66-68), and, where an empty row exists, the row execute_move fills first (BinPackingLogic.py:103-105).
    If no row of the window is empty, t = H - 1: the reference's `for` falls through.  Such moves exist, legality only counts cells
    (BinPackingLogic.py:89).  So 1 <= H - t <= H: a move that lands low weighs more.
  - Limits: w_pow, h_pow, land_pow >= 0, w_pow + h_pow <= 2, land_pow <= 2.  Then 1 <= u <= 4096 * 4096 = 2^24, which float32
    holds exactly, and T = sum of u over all legal moves <= 8192 * 2^24 = 2^37: a 64-bit integer sum, whose value does not depend
    on the summation order.
  - pi[a] = float32(float64(u) / float64(T)) at the legal actions a = i * W + c -- one IEEE double division, rounded once to
    float32 -- and 0.0f everywhere else.  A state without a legal move gives an all-zero row.
  - With (0, 0, 0) the row is float32(1) / float32(W * N) in every entry, bit for bit what it was before the prior existed.
"""
import functools

import numpy as np

import evaluators as ev
import oracle_lib as orc
import playout_policy_ref as pp
import rollout_ref as rr

UNIFORM = (0, 0, 0)
NAMES = {"uniform": (0, 0, 0), "low": (0, 0, 1), "low2": (0, 0, 2), "width2": (2, 0, 0), "area": (1, 1, 0), "width2-low2": (2, 0, 2)}


def check(prior):
    w_pow, h_pow, land_pow = prior
    assert w_pow >= 0 and h_pow >= 0 and land_pow >= 0 and w_pow + h_pow <= 2 and land_pow <= 2
    return int(w_pow), int(h_pow), int(land_pow)


def has_empty_row(board, c, w):
    return any(not board[r, c:c + w].any() for r in range(board.shape[0]))


def landing_row(board, c, w):
    """t: the first row whose window [c, c + w) is empty, H - 1 if none is (BinPackingLogic.py:66-68)."""
    H = board.shape[0]
    for r in range(H):
        if not board[r, c:c + w].any():
            return r
    return H - 1


def weights(W, H, N, board, rem, wh, prior):
    """u of every action -> list of A Python ints, 0 at the illegal actions."""
    w_pow, h_pow, land_pow = check(prior)
    board = np.asarray(board, np.uint8).reshape(H, W)
    mask, _ = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], np.asarray(rem, np.uint8))
    u = [0] * (W * N)
    for a in np.flatnonzero(mask):
        i, c = divmod(int(a), W)
        w, h = int(wh[i, 0]), int(wh[i, 1])
        u[a] = w ** w_pow * h ** h_pow * (H - landing_row(board, c, w)) ** land_pow
    return u


def prior_row(W, H, N, board, rem, wh, prior):
    """-> float32 [A]."""
    A = W * N
    if check(prior) == UNIFORM:
        return np.full(A, np.float32(1) / np.float32(A), dtype=np.float32)
    u = weights(W, H, N, board, rem, wh, prior)
    T = sum(u)  # a Python integer: exact
    assert T <= 2 ** 37
    row = np.zeros(A, np.float32)
    for a, x in enumerate(u):
        if x:
            row[a] = np.float32(np.float64(x) / np.float64(T))
    return row


def evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=pp.UNIFORM, prior=UNIFORM):
    """Closure with OracleMCTS's eval_py signature: (board, rem) -> (pi float32 [A], v float32 [1])."""
    def eval_py(board, rem):
        total = sum(pp.playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j, policy=policy)[0] for j in range(playouts))
        return prior_row(W, H, N, board, rem, wh, prior), np.array([np.float32(total) / np.float32(playouts)], dtype=np.float32)
    return eval_py


def oracle(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=pp.UNIFORM, prior=UNIFORM):
    """OracleMCTS of one instance whose evaluator is the restatement under (policy, prior); begin_episode done."""
    m = orc.OracleMCTS(W, H, N, 1.0, rr.ALPHA, evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy, prior),
                       lambda b, r: ev.tie_value(ev.pack_board(b), r, tie_salt))
    m.begin_episode(wh[:, 0], wh[:, 1], area, buf)
    return m


# ---- the states of the GPU parity test: shared with the CPU test that proves what they reach ------------------------------------------------
GPU_SEED, GPU_SALT = pp.GPU_SEED, pp.GPU_SALT
GPU_PRIORS = ((0, 0, 1), (0, 0, 2), (2, 0, 0), (1, 1, 1), (2, 0, 2))
PRIOR_B = (0, 2, 2)  # on state B in addition: T = 2^36
GEOMETRIES = dict(rr.GEOMETRIES)
GEOMETRIES["4x4/2"] = (4, 4, 2, "hand")  # state A's


def state_a():
    """W = H = 4, N = 2, items (2, 1) and (1, 1), cell (r, r % 2) set in every row: action 0 is legal and its window has no empty row."""
    board = np.zeros((4, 4), np.uint8)
    for r in range(4):
        board[r, r % 2] = 1
    wh = np.array([[2, 1], [1, 1]], np.uint8)
    return wh, 3, board, np.ones(2, np.uint8), 5007


def state_b():
    """W = H = 64, N = 128, every item (1, 64), row 0 set in the even columns: 4 096 legal moves, T = 2^36 under (0, 2, 2)."""
    board = np.zeros((64, 64), np.uint8)
    board[0, 0::2] = 1
    wh = np.tile(np.array([1, 64], np.uint8), (128, 1))
    return wh, 128 * 64, board, np.ones(128, np.uint8), 6007


@functools.lru_cache(maxsize=None)
def gpu_states(name):
    """The chosen states of geometry `name` -> list of (item sizes, area, board, rem, episode id): playout_policy_ref's three where the
    geometry is one of rollout_ref's, then the hand-built state of the geometry."""
    out = list(pp.gpu_states(name)) if name in rr.GEOMETRIES else []
    if name == "4x4/2":
        out.append(state_a())
    if name == "64x64/128":
        out.append(state_b())
    return out


def gpu_priors(name, k):
    """The priors state k of geometry `name` is checked under."""
    return GPU_PRIORS + ((PRIOR_B,) if name == "64x64/128" and k == len(gpu_states(name)) - 1 else ())


# ---- the whole-search cases ----------------------------------------------------------------------------------------------------------------------
PRIOR_SEARCH, POLICY_SEARCH = (2, 0, 2), (2, 0)
SEARCH_SIMS, SEARCH_K = 24, 3
# geometry -> (moves after whose search the comparison stops, None = the whole episode; seed of the instance)
SEARCH_CASES = {"10x10/8": (None, 0), "12x12/70": (3, 0), "40x6/12": (2, 0)}


def search_instance(name):
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area = rr.make_items(name, np.random.default_rng(SEARCH_SIMS + N + 1000 * SEARCH_CASES[name][1]))
    return wh, area, rr.BUFFERS["zeros"] if name == "12x12/70" else rr.BUFFERS["mixed"], 4100 + N


@functools.lru_cache(maxsize=None)
def first_root_counts(name, prior):
    """The oracle's root counts of the first searched move of search_instance(name) under `prior`."""
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, buf, eid = search_instance(name)
    m = oracle(W, H, N, wh, area, buf, GPU_SEED, GPU_SALT, eid, SEARCH_K, POLICY_SEARCH, prior)
    c = m.action_counts(np.zeros((H, W), np.uint8), np.ones(N, np.uint8), SEARCH_SIMS)
    m.close()
    return c
