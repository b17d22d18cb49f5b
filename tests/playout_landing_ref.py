"""Python restatement of the playouts' landing power (include/rp_engine.h: rp_set_playout_landing) over the oracle's rules.  Test
infrastructure: integer arithmetic and the oracle's C functions only, so the HIP kernels can be held to it bit for bit.  It parallels
playout_policy_ref.playout_path / playout / evaluator / oracle with one more argument, land_pow; the stream, the ranking and the tie rule
are rollout_ref's, the item weights playout_policy_ref's, the landing row rollout_prior_ref's.

The sampling rule, as the header states it.  At step s of playout j, on the playout's current board:
  - m_i is the legal-column mask of item i.  No legal move ends the playout.
  - wt_i = w_i^w_pow * h_i^h_pow, from the playout policy.
  - L(i, c) = (H - t(w_i, c))^land_pow, t(w, c) the first row whose window [c, c + w) is empty, H - 1 if none is.  1 <= L <= 4096.
  - R_i = sum of L(i, c) over c in m_i <= 2^18, S_i = wt_i * R_i <= 2^30, T = sum S_i <= 2^37.
  - pick = umulhi(sample(h0, j, s), T), the same stream: h0 = mix64(key_hash(S, seed) ^ e).
  - item = the first i whose inclusive sum of S exceeds pick; q = floor((pick - sum_{k<i} S_k) / wt_i) < R_i; column = the first legal
    column c of the item, ascending, whose inclusive sum of L(i, .) over the item's legal columns up to c exceeds q.
  - With land_pow == 0 this is playout_policy_ref's rule, bit for bit.
"""
import functools

import numpy as np

import evaluators as ev
import oracle_lib as orc
import playout_policy_ref as pp
import rollout_prior_ref as rp
import rollout_ref as rr


def check(land_pow):
    assert isinstance(land_pow, int) and 0 <= land_pow <= 2
    return land_pow


def landing_rows(board, w):
    """rollout_prior_ref.landing_row(board, c, w) of every column c at once -> int [W] (windows that leave the board are clipped, as
    the slice there is).  pick_move holds the row of every move it picks to landing_row itself."""
    H, W = board.shape
    cs = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(board != 0, axis=1, dtype=np.int64)], axis=1)
    empty = (cs[:, np.minimum(np.arange(W) + w, W)] - cs[:, :W]) == 0  # [H, W]: row r's window at column c is empty
    return np.where(empty.any(axis=0), empty.argmax(axis=0), H - 1)


def pick_move(mask, W, N, wt, x, board, wh, land_pow):
    """The move that draw x chooses among the legal moves of `mask` (uint8 [N * W]) on `board` ([H, W] cells) -> (action, dict of the
    step: T, pick, item, q, R = R_item, wt, bit = the column's number among the item's legal columns, c = the item's legal columns,
    rows = the landing rows of the item's legal columns, last = the pick fell in the last item that has a legal move)."""
    mask = np.asarray(mask).reshape(N, W)
    H = board.shape[0]
    cols = [[int(c) for c in np.flatnonzero(mask[i])] for i in range(N)]
    t_of = {w: landing_rows(board, w) for w in {int(wh[i, 0]) for i in range(N) if cols[i]}}  # items of one width share their landing rows
    rows = [[int(t_of[int(wh[i, 0])][c]) for c in cols[i]] for i in range(N)]
    L = [[(H - t) ** land_pow for t in rows[i]] for i in range(N)]
    S = [wt[i] * sum(L[i]) for i in range(N)]
    T = sum(S)
    assert 0 < T <= 1 << 37 and max(S) <= 1 << 30
    pick = rr.umulhi(x, T)
    before = 0
    for i in range(N):
        if before + S[i] > pick:
            break
        before += S[i]
    q = (pick - before) // wt[i]
    assert q < sum(L[i])
    run = 0
    for bit, l in enumerate(L[i]):
        run += l
        if run > q:
            break
    assert rows[i][bit] == rp.landing_row(board, cols[i][bit], int(wh[i, 0]))
    last = max(k for k in range(N) if cols[k])
    return i * W + cols[i][bit], dict(T=T, pick=pick, item=i, q=q, R=sum(L[i]), wt=wt[i], bit=bit, c=len(cols[i]), rows=rows[i], last=i == last,
                                      in_last_span=len(cols[i]) > 1 and bit == len(cols[i]) - 1)


def playout_path(W, H, N, board, rem, wh, seed, episode_id, j, trace=None, policy=pp.UNIFORM, land_pow=0):
    """Plays playout j from (board [H, W] cells, rem [N]) under (policy, land_pow) -> (moves, final board, final rem).  trace: a list that
    receives (legal-move mask, nv, draw x, action, step dict of pick_move, board before the move) of every step."""
    check(land_pow)
    board = np.array(board, np.uint8).reshape(H, W).copy(); rem = np.array(rem, np.uint8).copy()
    iw, ih = wh[:, 0], wh[:, 1]
    wt = pp.weights(wh, policy)
    h0 = ev.splitmix64(ev.key_hash(ev.pack_board(board), rem, seed) ^ (int(episode_id) & ev.M64))
    moves = 0
    for s in range(N):  # every move places one item
        mask, nv = orc.valid_moves(W, H, N, board, iw, ih, rem)
        if nv == 0:
            break
        x = orc.lib().orc_sample_u64(h0, int(j), s)
        a, step = pick_move(mask, W, N, wt, x, board, wh, land_pow)
        if trace is not None:
            trace.append((mask, int(nv), int(x), a, step, board.copy()))
        rc, board, rem = orc.next_state(W, H, N, board, iw, ih, rem, a)
        assert rc == 0
        moves += 1
    return moves, board, rem


def playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j, policy=pp.UNIFORM, land_pow=0):
    """-> (outcome, score, moves, final rows uint64 [H])."""
    moves, fb, fr = playout_path(W, H, N, board, rem, wh, seed, episode_id, j, policy=policy, land_pow=land_pow)
    e, r = rr.rank(W, H, fb, fr, area, int(wh[:, 1].max()), buf, tie_salt)
    return e, r, moves, ev.pack_board(fb)


def evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=pp.UNIFORM, land_pow=0, prior=rp.UNIFORM):
    """Closure with OracleMCTS's eval_py signature: (board, rem) -> (pi float32 [A], v float32 [1]); pi is rollout_prior_ref's row."""
    def eval_py(board, rem):
        total = sum(playout(W, H, N, board, rem, wh, area, buf, seed, tie_salt, episode_id, j, policy=policy, land_pow=land_pow)[0] for j in range(playouts))
        return rp.prior_row(W, H, N, board, rem, wh, prior), np.array([np.float32(total) / np.float32(playouts)], dtype=np.float32)
    return eval_py


def oracle(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy=pp.UNIFORM, land_pow=0, prior=rp.UNIFORM):
    """OracleMCTS of one instance whose evaluator is the restatement under (policy, land_pow, prior); begin_episode done."""
    m = orc.OracleMCTS(W, H, N, 1.0, rr.ALPHA, evaluator(W, H, N, wh, area, buf, seed, tie_salt, episode_id, playouts, policy, land_pow, prior),
                       lambda b, r: ev.tie_value(ev.pack_board(b), r, tie_salt))
    m.begin_episode(wh[:, 0], wh[:, 1], area, buf)
    return m


def under(monkeypatch, policy, land_pow):
    """For the duration of a test, rollout_ref's playout functions are the ones above under (policy, land_pow): best_playout_ref.episode
    calls them by name, and with this it computes the incumbent of a search whose playouts follow the setting."""
    for name in ("playout_path", "playout", "evaluator", "oracle"):
        monkeypatch.setattr(rr, name, functools.partial(globals()[name], policy=policy, land_pow=land_pow))


# ---- the states of the GPU parity test: shared with the CPU test that proves what they reach ------------------------------------------------
GPU_SEED, GPU_SALT = pp.GPU_SEED, pp.GPU_SALT
GPU_SETTINGS = (((0, 0), 1), ((0, 0), 2), ((2, 0), 2), ((1, 1), 1), ((0, 2), 2))  # (policy, land_pow)
SETTING_B = ((0, 2), 2)  # state B is played under this one alone: T near 2^36
GPU_PLAYOUTS = 4
GEOMETRIES = rp.GEOMETRIES  # rollout_ref's and state A's 4x4/2


@functools.lru_cache(maxsize=None)
def gpu_states(name):
    """-> list of (item sizes, area, board, rem, episode id): playout_policy_ref's three states of a rollout_ref geometry (one only at
    64x64/128), then the hand-built state of the geometry (rollout_prior_ref.state_a / state_b)."""
    out = []
    if name in rr.GEOMETRIES:
        out = list(pp.gpu_states(name))
        if name == "64x64/128":
            out = out[1:2]  # the mid-game state
    if name == "4x4/2":
        out.append(rp.state_a())
    if name == "64x64/128":
        out.append(rp.state_b())
    return out


def gpu_settings(name, k):
    """The settings state k of geometry `name` is played under."""
    return (SETTING_B,) if name == "64x64/128" and k == len(gpu_states(name)) - 1 else GPU_SETTINGS


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's playouts of gpu_states(name), computed once -> {(setting, state, playout): (moves, final board cells, final
    rem, action list, trace)}."""
    W, H, N, _ = GEOMETRIES[name]
    out = {}
    for b, s in enumerate(gpu_states(name)):
        for setting in gpu_settings(name, b):
            for j in range(GPU_PLAYOUTS):
                trace = []
                m, fb, fr = playout_path(W, H, N, s[2], s[3], s[0], GPU_SEED, s[4], j, trace=trace, policy=setting[0], land_pow=setting[1])
                out[(setting, b, j)] = (m, fb, fr, [t[3] for t in trace], trace)
    return out


# ---- the whole-search cases: rollout_prior_ref's instances ------------------------------------------------------------------------------------
SEARCH_SETTING = ((2, 0), 2)
SEARCH_PRIOR = (2, 0, 2)
SEARCH_SIMS, SEARCH_K, SEARCH_CASES = rp.SEARCH_SIMS, rp.SEARCH_K, rp.SEARCH_CASES
search_instance = rp.search_instance
