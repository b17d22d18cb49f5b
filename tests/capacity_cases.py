"""The seeded instances of the capacity tests and their oracle references, shared by test_arena_ref_cpu.py (which checks that the
instances have the properties the GPU tests rely on) and test_gpu_capacity.py.  Every reference is computed once per process."""
import functools

import numpy as np

import arena_ref
import evaluators as ev
import oracle_lib as orc

KIND, SALT = "hashed", 7
BUF = (0.9, 0.8, 1.0, 0.85, 0.75)
PCHUNK_MIN, VCHUNK_MIN = 4096, 1024  # the engine's chunk sizes for W * N below them; the GPU tests read the real ones from rp_arena_peak

# (W, H, N, height of the rectangle that is split into the items, seed).  A split of the bin itself packs completely, so its search
# reaches every level; the items of a taller rectangle do not all fit, the episode ends early and its arenas open fewer chunks.
SMALL = (10, 10, 8, 48)  # W, H, N, simulations per move
SINGLE = (10, 10, 8, 10, 2)
RECLAIM = (10, 10, 8, 10, 6)
WIDE = (33, 12, 9, 12, 4)  # 64-bit rows
WIDE_SIMS = 40
ISOLATION = [(10, 10, 8, 18, 4), (10, 10, 8, 14, 6), (10, 10, 8, 10, 2), (10, 10, 8, 22, 2), (10, 10, 8, 18, 6)]  # the neediest in the middle
NEEDIEST = 2
RECOVERY = [3, 4, 0, 1, 0]  # indices into ISOLATION: what each slot plays after the failure, all of them instances that fit
TINY = (4, 3, 3, 2)  # the ring test's board: W, H, N, simulations per move
TINY_DISTINCT = 8
RING_SLOTS = 16
RING_CAP = max(4 * RING_SLOTS, 1024)  # the finished-episode ring of a context with RING_SLOTS slots (rp_engine.h)
RING_POOL = RING_CAP + 6
REPLAY_SIMS = 12
# the last two episodes end differently and have as many moves: with one example too few, the last move of the last episode is the one
# that does not fit, and the example of the same move of the episode before it is the one a stale index would point at
REPLAY_POOL = [(10, 10, 8, 10, s) for s in (11, 13, 14, 15, 12, 16)]


def split_items(W, H, N, split_h, seed):
    """Guillotine split of the W x split_h rectangle into N items like ItemsGenerator (BinPackingGame.py:257-285), every item within
    the W x H bin -> uint8 [N, 2] (w, h)."""
    for attempt in range(10000):  # the first split of this seed whose items all fit the bin
        rng = np.random.default_rng([seed, attempt])
        items = [(W, split_h)]
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
        if max(h for _, h in items) <= H:
            return np.array(items, np.uint8)
    raise RuntimeError("no split of %dx%d into %d items fits a %dx%d bin" % (W, split_h, N, W, H))


def items_of(inst):
    W, H, N, split_h, seed = inst
    return split_items(W, H, N, split_h, seed)


def tiny_instances():
    """TINY_DISTINCT different instances of the TINY board."""
    W, H, N, _ = TINY
    out, seen, seed = [], set(), 0
    while len(out) < TINY_DISTINCT:
        wh = split_items(W, H, N, H, seed)
        seed += 1
        if wh.tobytes() not in seen:
            seen.add(wh.tobytes()); out.append(wh)
    return np.stack(out)


def new_oracle(W, H, N, kind=KIND, salt=SALT):
    A = W * N
    return orc.OracleMCTS(W, H, N, 1.0, 0.75, lambda b, r: ev.table_eval(kind, ev.pack_board(b), r, A, salt),
                          lambda b, r: ev.tie_value(ev.pack_board(b), r, salt))


def replay_moves(W, H, N, wh, actions):
    """The oracle's rules over an action list -> (filled-row mask per move, final bin rows u64 [H])."""
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    filled = []
    for a in actions:
        rc, nb, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, int(a))
        filled.append(sum(1 << r for r in range(H) if not np.array_equal(nb[r], board[r])))
        board = nb
    return filled, ev.pack_board(board)


def _describe(m, W, H, N, wh, moves_at=None):
    """The finished oracle's tree as the arena model sees it."""
    dump = m.dump()

    def n_valid_of(rows, rem):
        board = ev.unpack_board(np.frombuffer(rows, np.uint64), W)
        return orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], np.frombuffer(rem, np.uint8))[1]

    nodes = arena_ref.tree_nodes(dump, n_valid_of)
    pchunk, vchunk = max(PCHUNK_MIN, W * N), max(VCHUNK_MIN, W * N)
    offs, P = arena_ref.prior_layout(nodes, pchunk)
    d = dict(dump=dump, keys=list(dump.keys()), nodes=nodes, n_nodes=len(nodes), offsets=offs, P=P, visited=arena_ref.visited_bounds(nodes, vchunk))
    if moves_at is not None:
        d["moves_at"] = moves_at
        d["P_reclaim"] = arena_ref.prior_layout(nodes, pchunk, moves=moves_at)[1]
    return d


@functools.lru_cache(maxsize=None)
def auto_episode(inst, sims, kind=KIND, salt=SALT):
    """One episode with the lowest-index argmax move rule (RP_MOVE_ARGMAX_FIRST) -> dict: actions, outcome, score, the tree and what
    the arena model makes of it."""
    W, H, N = inst[:3]
    wh = items_of(inst)
    m = new_oracle(W, H, N, kind, salt)
    m.begin_episode(wh[:, 0], wh[:, 1], W * H, BUF)
    actions, counts, outcome, score = m.play_episode(sims, policy=0)
    d = _describe(m, W, H, N, wh)
    m.close()
    filled, board = replay_moves(W, H, N, wh, actions)
    d.update(actions=[int(a) for a in actions], counts=counts, outcome=outcome, score=score, wh=wh, filled=filled, board=board)
    return d


@functools.lru_cache(maxsize=None)
def external_episode(inst, sims):
    """The same episode driven move by move (getActionProb on successive states of one MCTS object), with the root's visit counts
    before every move and the number of nodes after it: the interleaving of node creation and moves that reclaim depends on."""
    W, H, N = inst[:3]
    wh = items_of(inst)
    m = new_oracle(W, H, N)
    m.begin_episode(wh[:, 0], wh[:, 1], W * H, BUF)
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    counts, actions, moves_at = [], [], []
    while True:
        c = m.action_counts(board, rem, sims)
        if not c.any():
            break
        counts.append(c)
        actions.append(int(np.argmax(c)))
        _, board, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, actions[-1])
        moves_at.append(int(m.stats()["nodes"]))  # the child of a visited move exists already: the move creates nothing
        if not orc.has_valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem):
            break
    d = _describe(m, W, H, N, wh, moves_at)
    m.close()
    d.update(actions=actions, counts=counts, wh=wh)
    return d


# A level whose runs fill a chunk to its last entry.  65 unit squares on a 4-wide board: the empty bin has one legal column, a bin with
# one square has two, so the root has 65 legal moves and each of its children 64 * 2 = 128.  Under the uniform evaluator (equal
# priors, v = 0) an unvisited move outscores every visited one, so every simulation after the first (which expands the root) opens
# another child of the root: 39 runs of 128 entries at level 1, the 32nd of which ends exactly at the chunk's end (32 * 128 = 4096).
EXACT_FILL = (4, 17, 65, 40)  # W, H, N, simulations


@functools.lru_cache(maxsize=None)
def exact_fill_search():
    W, H, N, sims = EXACT_FILL
    wh = np.ones((N, 2), np.uint8)
    m = new_oracle(W, H, N, "uniform", SALT)
    m.begin_episode(wh[:, 0], wh[:, 1], N, BUF)
    counts = m.action_counts(np.zeros((H, W), np.uint8), np.ones(N, np.uint8), sims)
    d = _describe(m, W, H, N, wh)
    m.close()
    d.update(counts=counts, wh=wh)
    return d


@functools.lru_cache(maxsize=None)
def tiny_episodes():
    W, H, N, sims = TINY
    out = []
    for wh in tiny_instances():
        m = new_oracle(W, H, N)
        m.begin_episode(wh[:, 0], wh[:, 1], W * H, BUF)
        actions, _, outcome, score = m.play_episode(sims, policy=0, want_counts=False)
        m.close()
        filled, board = replay_moves(W, H, N, wh, actions)
        out.append(dict(wh=wh, actions=[int(a) for a in actions], outcome=outcome, score=score, filled=filled, board=board))
    return out
