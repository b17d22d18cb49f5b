"""CPU checks of the exact sequential ranked-reward buffer (resource_packing_self_play_amd/rank_buffer.py): prefix thresholds
against the reference's formula, threshold classes against a brute-force ranked outcome, the speculate-and-repair loop against the
literal sequential loop with a fake deterministic player, and the rank sharding of a round's plan."""
import numpy as np
import pytest

from resource_packing_self_play_amd import rank_buffer as rb


def literal_threshold(buf, alpha):
    """BinPackingGame.getRankedReward's threshold, verbatim (BinPackingGame.py:203-206)."""
    if len(buf) == 0:
        return False, 0.0
    s = np.sort(buf)
    return True, float(s[int(np.floor(len(s) * alpha)) - 1])


def literal_prefix(buf0, scores, alpha):
    buf = list(buf0)
    out = []
    for x in scores:
        out.append(literal_threshold(buf, alpha))
        buf.append(float(x))
    return out


SCORE_POOL = np.array([0.0, 0.5, 0.6, 0.625, 2 / 3, 0.7, 0.75, 0.8, 0.8125, 5 / 6, 0.9, 1.0])


@pytest.mark.parametrize("alpha", [0.75, 0.5, 0.25, 1.0, 0.1, 0.0])
@pytest.mark.parametrize("n0", [0, 1, 2, 3, 4, 7, 8, 100])
def test_prefix_thresholds_match_the_literal_formula(alpha, n0):
    rng = np.random.default_rng(1000 * n0 + int(alpha * 100))
    for trial in range(6):
        E = int(rng.integers(1, 60))
        pool = SCORE_POOL if trial % 2 else rng.random(8)  # heavy ties / few distinct values, or continuous
        buf0 = list(rng.choice(pool, n0))
        scores = rng.choice(pool, E)
        bl, has = rb.prefix_thresholds(buf0, scores, alpha)
        ref = literal_prefix(buf0, scores, alpha)
        assert [bool(h) for h in has] == [h for h, _ in ref]
        for k, (h, b) in enumerate(ref):
            if h:
                assert bl[k] == b, (k, bl[k], b)


def test_prefix_threshold_wrap_and_integer_quantiles():
    # length 1: floor(0.75) - 1 = -1 -> the largest (the only) value; length 4, alpha 0.75: floor(3.0) - 1 = 2 exactly
    bl, has = rb.prefix_thresholds([], [0.5, 0.9, 0.2, 0.7, 0.3], 0.75)
    assert list(has) == [False, True, True, True, True]
    assert bl[1] == 0.5 and bl[2] == 0.5 and bl[3] == 0.5 and bl[4] == 0.7
    bl, has = rb.prefix_thresholds([0.4], [0.1], 0.75)
    assert bl[0] == 0.4  # wrap -> max
    assert rb.threshold([0.2, 0.9, 0.5, 0.7], 0.75) == (True, 0.7)


def test_prefix_thresholds_large_pool_is_fast_and_exact():
    import time
    rng = np.random.default_rng(7)
    buf0 = list(rng.choice(SCORE_POOL, 100))
    scores = rng.choice(SCORE_POOL, 8 * 32768)
    t0 = time.time()
    bl, has = rb.prefix_thresholds(buf0, scores, 0.75)
    assert time.time() - t0 < 20.0
    assert has.all()
    for k in (0, 1, 17, 4096, 100000, len(scores) - 1):  # spot checks against the literal formula
        assert bl[k] == literal_threshold(buf0 + list(scores[:k]), 0.75)[1]


def brute_outcomes(R_row, has, bl):
    return tuple(rb.ranked_outcome(float(r), has, bl) for r in R_row)


def test_reachable_scores_are_the_device_arithmetic():
    R = rb.reachable_scores([100, 37], [4, 9], 10, 12)
    assert R.shape == (2, 13)
    assert R[0, 0] == 0.0 and R[0, 10] == 1.0 and R[0, 11] == 10.0 / 11.0 and R[0, 1] == 0.0  # b = 10: t < 10 unreachable
    assert R[1, 9] == 1.0 and R[1, 12] == 9.0 / 12.0  # b = max(ceil(3.7), 9) = 9
    sup = rb.superset_scores(12)
    for row in R:
        assert set(row.tolist()) <= set(sup.tolist())


@pytest.mark.parametrize("per_instance", [True, False])
def test_class_keys_equal_iff_the_ranked_outcomes_are_equal(per_instance):
    rng = np.random.default_rng(3 if per_instance else 4)
    W, H = 10, 12
    E = 40
    area = rng.integers(20, W * H + 1, E)
    max_h = rng.integers(1, H + 1, E)
    R = rb.reachable_scores(area, max_h, W, H)
    Rk = R if per_instance else rb.superset_scores(H)
    sup = rb.superset_scores(H)
    cands = np.concatenate([sup, (sup[:-1] + sup[1:]) / 2, [-1.0, 1.5]])  # every reachable value, every gap, out of range
    for trial in range(30):
        bl = rng.choice(cands, E)
        has = rng.random(E) < 0.85
        bl2 = rng.choice(cands, E)
        has2 = rng.random(E) < 0.85
        k1 = rb.class_keys(bl, has, Rk)
        k2 = rb.class_keys(bl2, has2, Rk)
        for e in range(E):
            same = brute_outcomes(R[e], has[e], bl[e]) == brute_outcomes(R[e], has2[e], bl2[e])
            if per_instance:
                assert (k1[e] == k2[e]) == same, (e, bl[e], bl2[e])
            elif k1[e] == k2[e]:  # the superset's classes are finer: equal keys still mean equal play
                assert same


def make_player(R, salt, pool):
    """score = f(episode, class): a deterministic stand-in for a whole episode that depends on the threshold only through the class."""
    def f(e, key):
        h = (e * 0x9E3779B97F4A7C15 + int(key) * 0xBF58476D1CE4E5B9 + salt) & ((1 << 64) - 1)
        h ^= h >> 29
        return float(pool[h % len(pool)])
    return f


def sequential_reference(buf0, E, alpha, R, f):
    buf = list(buf0)
    out = []
    for e in range(E):
        h, b = literal_threshold(buf, alpha)
        key = rb.class_keys([b], [h], R[e:e + 1] if R.ndim == 2 else R)[0]
        out.append(f(e, key))
        buf.append(out[-1])
    return np.array(out)


def batched_repair(buf0, E, alpha, R, f):
    h0, b0 = rb.threshold(buf0, alpha)
    k0 = rb.class_keys(np.full(E, b0), np.full(E, h0), R)
    spec = np.array([f(e, k0[e]) for e in range(E)])

    def play(idx, bl, has):
        keys = rb.class_keys(bl, has, R[idx] if R.ndim == 2 else R)
        return [f(int(e), k) for e, k in zip(idx, keys)]
    return rb.repair(buf0, spec, alpha, R, play)


@pytest.mark.parametrize("case", range(60))
def test_repair_equals_the_literal_sequential_loop(case):
    rng = np.random.default_rng(case)
    W, H = 10, int(rng.integers(6, 16))
    E = int(rng.integers(1, 80))
    alpha = float(rng.choice([0.75, 0.5, 0.9, 0.25]))
    area = rng.integers(W * 2, W * H + 1, E)
    max_h = rng.integers(1, H + 1, E)
    R = rb.reachable_scores(area, max_h, W, H) if case % 3 else rb.superset_scores(H)
    pool = np.unique(rb.reachable_scores(area, max_h, W, H))
    n0 = int(rng.choice([0, 0, 1, 2, 5, 30]))
    buf0 = list(rng.choice(pool, n0))
    f = make_player(R, case, pool)
    res = batched_repair(buf0, E, alpha, R, f)
    ref = sequential_reference(buf0, E, alpha, R, f)
    assert np.array_equal(res["scores"], ref)
    assert res["rounds"] <= E and len(res["replayed"]) == res["rounds"]
    lit = literal_prefix(buf0, ref, alpha)
    for e, (h, b) in enumerate(lit):
        assert bool(res["has_buf"][e]) == h and (not h or res["bl"][e] == b)


def test_repair_adversarial_cascade_terminates_within_E_rounds():
    """Every episode's score flips with its class, and each class depends on the previous score: the worst case replays a chain."""
    E, H = 40, 8
    R = rb.superset_scores(H)
    lo, hi = 0.5, 1.0

    def f(e, key):  # below / at the threshold -> low score, above -> high: the running 75 % quantile keeps moving
        return hi if key % 4 == 0 else lo
    res = batched_repair([], E, 0.75, R, f)
    ref = sequential_reference([], E, 0.75, R, f)
    assert np.array_equal(res["scores"], ref)
    assert res["rounds"] <= E


def test_shard_plan_with_a_fake_all_gather_covers_the_round():
    rng = np.random.default_rng(11)
    for world in (1, 2, 3, 5):
        for n in (0, 1, 4, 17):
            idx = np.sort(rng.choice(1000, n, replace=False))
            parts = [rb.shard_plan(idx, r, world) for r in range(world)]
            assert np.array_equal(np.concatenate(parts) if parts else np.zeros(0), idx)  # the all-gather in rank order = the plan
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


def test_repair_with_sharded_rounds_equals_one_rank():
    """Each round: every rank plays its block of the plan, an all-gather (here: concatenation in rank order) returns all scores."""
    rng = np.random.default_rng(5)
    W, H, E = 10, 10, 50
    area = rng.integers(30, 101, E); max_h = rng.integers(1, 11, E)
    R = rb.reachable_scores(area, max_h, W, H)
    f = make_player(R, 99, np.unique(R))
    one = batched_repair([], E, 0.75, R, f)
    for world in (2, 3):
        h0, b0 = rb.threshold([], 0.75)
        k0 = rb.class_keys(np.full(E, b0), np.full(E, h0), R)
        spec = np.array([f(e, k0[e]) for e in range(E)])

        def play(idx, bl, has):
            keys = dict(zip(idx.tolist(), rb.class_keys(bl, has, R[idx]).tolist()))
            gathered = {}
            for r in range(world):
                mine = rb.shard_plan(idx, r, world)
                gathered.update({int(e): f(int(e), keys[int(e)]) for e in mine})
            return [gathered[int(e)] for e in idx]
        res = rb.repair([], spec, 0.75, R, play)
        assert np.array_equal(res["scores"], one["scores"]) and res["replayed"] == one["replayed"]

