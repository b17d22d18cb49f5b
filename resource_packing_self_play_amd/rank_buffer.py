"""Exact sequential ranked-reward (R2) buffer for a batched iteration (NumPy only).

The reference plays an iteration's episodes one after another and appends each score to `rewards_list` right away
(xw_mcts/CoachBPP.py:123-134), so episode k is ranked against `buffer + scores[0..k-1]`.  The batched Coach plays them all at
once against the buffer as it stood when the iteration began (the snapshot).  This module turns the snapshot's results into the
sequential ones by speculate-and-repair:

  * an episode depends on the buffer only through its R2 threshold (has_buf, bl), and on that only through the outcome
    `ranked_reward` gives each score r the episode can reach -- r in {0} and {b / t : t = 1..H}, b = max(ceil(area / W), max_h)
    (BinPackingGame.py:196-212); that outcome vector is the episode's THRESHOLD CLASS (`class_keys`), and two thresholds of one
    class play the same episode;
  * from the scores of a round every episode's exact prefix threshold follows (`prefix_thresholds`); only the episodes whose class
    changed are replayed, with the same episode id (`repair`), until no class changes.  The lowest mismatching episode depends only
    on earlier, already final episodes, so it is final after its replay: the first mismatch moves up every round, at most E rounds.
"""
import heapq
import math

import numpy as np


def threshold(rewards, alpha):
    """(has_buf, bl) of one buffer: sorted(rewards)[int(floor(len * alpha)) - 1] with Python's -1 wrap (BinPackingGame.py:203-206);
    an index past the end is clamped like the engine's rank_threshold."""
    n = len(rewards)
    if n == 0:
        return False, 0.0
    s = sorted(float(x) for x in rewards)
    idx = int(math.floor(n * alpha)) - 1
    if idx < 0:
        idx += n
    return True, s[min(idx, n - 1)]


def prefix_thresholds(buf0, scores, alpha):
    """Thresholds of all E episodes of an iteration played in order: episode k is ranked against buf0 + scores[:k].
    -> (bl [E] float64, has_buf [E] bool).  Two heaps hold the running order statistic: O((len(buf0) + E) log(len(buf0) + E))."""
    buf0 = [float(x) for x in buf0]
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    E = scores.shape[0]
    bl = np.zeros(E, np.float64)
    has = np.zeros(E, bool)
    low = []  # max-heap (negated) of the `size` smallest values
    up = list(buf0)  # min-heap of the rest
    heapq.heapify(up)
    top = max(buf0) if buf0 else -math.inf  # the -1 wrap (floor(L * alpha) == 0) reads the largest value
    L = len(buf0)
    for k in range(E):
        if L > 0:
            want = min(int(math.floor(L * alpha)), L)
            while len(low) < want:
                heapq.heappush(low, -heapq.heappop(up))
            while len(low) > want:
                heapq.heappush(up, -heapq.heappop(low))
            has[k] = True
            bl[k] = -low[0] if want > 0 else top
        x = float(scores[k])
        if low and x < -low[0]:  # keep every value of `low` <= every value of `up`
            heapq.heappush(up, -heapq.heapreplace(low, -x))
        else:
            heapq.heappush(up, x)
        top = max(top, x)
        L += 1
    return bl, has


def reachable_scores(area, max_h, W, H):
    """[E, H + 1] float64: every score r an instance can end with -- 0 (an item left out) and b / t for the top row t = b..H, computed
    in double like the device (rp_engine.hip ranked_reward); entries for t < b (unreachable) are 0."""
    b = np.maximum(np.ceil(np.asarray(area, np.float64).reshape(-1) / float(W)), np.asarray(max_h, np.float64).reshape(-1))
    t = np.arange(1, int(H) + 1, dtype=np.float64)
    r = np.where(t[None, :] >= b[:, None], b[:, None] / t[None, :], 0.0)
    return np.concatenate([np.zeros((b.shape[0], 1)), r], axis=1)


def superset_scores(H):
    """{0} and {b / t : 1 <= b <= t <= H} sorted: every score of any instance on an H-row grid (episode-independent, exact, coarser
    only in that it may replay an episode whose own reachable scores did not cross the threshold)."""
    H = int(H)
    vals = [0.0] + [float(b) / float(t) for t in range(1, H + 1) for b in range(1, t + 1)]
    return np.unique(np.asarray(vals, np.float64))


def class_keys(bl, has_buf, R):
    """Threshold class of every episode as one int64: 2 * #{r in R : r < bl} + [bl in R] over the reachable scores R ([E, K] per
    episode or [K] shared) without r == 1 (always +1, BinPackingGame.py:207).  Equal keys of one episode <=> equal ranked outcome for
    every reachable score.  has_buf == 0 ranks everything +1, which is the key 0 (no score below or at bl)."""
    bl = np.asarray(bl, np.float64).reshape(-1)
    has = np.asarray(has_buf).reshape(-1) != 0
    R = np.asarray(R, np.float64)
    if R.ndim == 1:
        Rs = np.sort(R[R != 1.0])
        lo = np.searchsorted(Rs, bl, side="left")
        hi = np.searchsorted(Rs, bl, side="right")
        eq = hi > lo
    else:
        Rm = np.where(R == 1.0, np.nan, R)  # NaN compares false both ways
        lo = (Rm < bl[:, None]).sum(axis=1)
        eq = (Rm == bl[:, None]).any(axis=1)
    key = 2 * lo.astype(np.int64) + eq.astype(np.int64)
    return np.where(has, key, 0)


def ranked_outcome(r, has_buf, bl):
    """ranked_reward's outcome of score r: +1 / -1, or 2 for the r == bl tie (resolved by tie_value, independent of bl)."""
    if not has_buf or r > bl or r == 1.0:
        return 1
    return -1 if r < bl else 2


def repair(buf0, scores, alpha, R, play, played=None):
    """Speculate-and-repair: `scores` [E] were played against `played` = (bl [E], has_buf [E]) (default: the snapshot of buf0 for
    every episode).  play(index [n] int64, bl [n], has_buf [n]) -> new scores [n] replays those episodes with those thresholds.
    -> dict(scores, bl, has_buf (the exact prefix thresholds), rounds, replayed (episodes per round), keys_played (the class each
    episode's final play had)).  Terminates after at most E rounds (see the module docstring)."""
    scores = np.array(scores, dtype=np.float64).reshape(-1)
    E = scores.shape[0]
    if played is None:
        h0, b0 = threshold(buf0, alpha)
        played = (np.full(E, b0), np.full(E, h0))
    keys_played = class_keys(played[0], played[1], R)
    replayed = []
    while True:
        bl, has = prefix_thresholds(buf0, scores, alpha)
        keys = class_keys(bl, has, R)
        idx = np.nonzero(keys != keys_played)[0].astype(np.int64)
        if idx.size == 0:
            return dict(scores=scores, bl=bl, has_buf=has, rounds=len(replayed), replayed=replayed, keys_played=keys_played)
        if len(replayed) >= E:
            raise RuntimeError("rank-buffer repair did not converge in %d rounds" % E)
        scores[idx] = np.asarray(play(idx, bl[idx], has[idx]), dtype=np.float64).reshape(-1)
        keys_played[idx] = keys[idx]
        replayed.append(int(idx.size))


def shard_plan(index, rank, world):
    """The part of a round's replay list `index` that rank `rank` of `world` plays: a contiguous block, sizes differ by at most one
    (distributed.shard's cut)."""
    base, rem = divmod(len(index), int(world))
    lo = rank * base + min(rank, rem)
    return np.asarray(index[lo:lo + base + (1 if rank < rem else 0)], dtype=np.int64)
