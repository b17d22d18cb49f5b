"""What the inputs of tests/test_gpu_move_incumbent.py reach, proved from the reference alone (tests/move_incumbent_ref.py; no GPU).  These
are conditions on the chosen instances, not measurements of the engine: every branch of the rule RP_MOVE_INCUMBENT (include/rp_engine.h)
must be taken by some episode the GPU tests play.  All 32 episodes of best_ref.SHAPES run here (a few seconds), with the table evaluators
best_ref.KINDS, buffer best_ref.BUF, salt 9, tree terminals only; the figures in the comments are what they give."""
import functools

import numpy as np
import pytest

import best_ref as br
import move_incumbent_ref as mi


@functools.lru_cache(maxsize=None)
def probes(switch_at=0):
    """{(shape, game): episode} over best_ref.SHAPES."""
    return {(s, g): mi.probe(s, g, switch_at=switch_at)[1] for s, shape in enumerate(br.SHAPES) for g in range(shape[5])}


def first_followed(ref):
    return ref["followed"].index(True) if any(ref["followed"]) else None


def test_the_reference_without_the_rule_is_the_oracles_episode():
    """switch_at = NEVER is RP_MOVE_ARGMAX_FIRST: the played line and the final incumbent are best_ref.oracle_episode's (one
    orc_play_episode call), so searching one simulation at a time leaves the same episode."""
    for (s, g), ref in probes(mi.NEVER).items():
        W, H, bin_h, N, sims, games = br.SHAPES[s]
        wh = br.instances(W, bin_h, N, games)[g]
        played, outcome, score, best = br.oracle_episode(W, H, N, wh, W * bin_h, br.BUF, br.KINDS[g % 2], sims, br.ARGMAX_FIRST, br.SEED, g)
        assert (ref["actions"], ref["outcome"], ref["score"]) == (played, outcome, score), (s, g)
        assert not any(ref["followed"])
        inc = ref["best"]
        assert (inc["score"], inc["outcome"], inc["updates"]) == (best["score"], best["outcome"], best["updates"]), (s, g)
        assert np.array_equal(inc["rows"], best["rows"])
        br.check_actions(best, W, H, N, wh, inc["actions"], inc["prefix"], played, where="%d/%d" % (s, g))


def test_the_invariant_holds_in_every_episode():
    for key, ref in probes().items():
        mi.check_invariant(ref)
        for mv, (f, inc) in enumerate(zip(ref["followed"], ref["running"])):  # a followed move is the incumbent's next action
            if f:
                assert inc["score"] > 0 and inc["moves"] > mv and inc["actions"][:mv + 1] == ref["actions"][:mv + 1], key
        assert not ref["off_line"], key  # under the rule from the start, condition 4 never fails for a live incumbent


def test_the_probe_reaches_every_branch():
    rule, argmax = probes(), probes(mi.NEVER)
    differ = [k for k in rule if rule[k]["actions"] != argmax[k]["actions"]]
    assert len(differ) >= 16  # 20
    from_zero = [k for k, r in rule.items() if r["followed"][0]]
    assert from_zero == [(0, 4), (4, 2)]  # an incumbent found by the first move's search and followed from move 0
    later = [k for k, r in rule.items() if any(r["followed"]) and not r["followed"][0]]
    assert len(later) >= 10  # 23: the fallback first, the incumbent later
    replaced = [k for k, r in rule.items() if any(r["followed"]) and any(h["at"] > first_followed(r) for h in r["history"])]
    assert len(replaced) >= 5 and (1, 0) in replaced  # 13: a better incumbent found from a root the rule had led to
    assert [h["at"] for h in rule[(1, 0)]["history"]] == [1, 2, 6]
    # a score-0 incumbent (a packing that dropped an item) is in the record, is never followed and is replaced later
    zero_then_better = [k for k, r in rule.items() if r["history"][0]["score"] == 0 and r["best"]["score"] > 0]
    assert len(zero_then_better) >= 2 and {(0, 1), (2, 4), (4, 5)} <= set(zero_then_better)
    # ... and in one of them moves are played while it is held: condition 2 decides on the device, the others hold
    held = [(k, mv) for k in zero_then_better for mv, inc in enumerate(rule[k]["running"]) if inc is not None and inc["score"] == 0 and inc["moves"] > mv]
    assert [k for k, _ in held] == [(2, 4), (2, 4)] and not any(rule[(2, 4)]["followed"][mv] for _, mv in held)
    never = [k for k, r in rule.items() if r["best"]["score"] == 0]
    assert len(never) >= 3 and not any(any(rule[k]["followed"]) for k in never)  # 7 end with an incumbent of score 0
    higher = sum(rule[k]["score"] > argmax[k]["score"] for k in rule)
    lower = sum(rule[k]["score"] < argmax[k]["score"] for k in rule)
    assert higher >= 10 and lower == 0  # 16 played better, none worse
    assert sum(r["n_followed"] for r in rule.values()) > 0


@pytest.mark.parametrize("kind,moves", [("hashed", [66, 67, 68, 69]), ("uniform", [68, 69])])
def test_more_than_64_items_follow_past_move_64(kind, moves):
    """The prefix comparison of a move index >= 64 is made by the second pair of lanes."""
    ref = mi.big_episode(kind)
    mi.check_invariant(ref)
    assert len(ref["actions"]) == mi.BIG_N and [mv for mv, f in enumerate(ref["followed"]) if f] == moves


SWITCHES = [(0, 1, 6), (1, 0, 3), (0, 4, 4), (2, 4, 5)]  # (shape, game, switch_at); the GPU test plays the same


def test_the_switch_instances():
    """Under RP_MOVE_ARGMAX_FIRST the played line left the incumbent's: at the switch the record holds an incumbent that scores above 0
    and has a next action, but its line does not pass through the root.  The rule keeps falling back there (no better incumbent arrives
    in these three, so the line is RP_MOVE_ARGMAX_FIRST's to the end).  The fourth switches while the line still passes through the
    root, and follows from the switch on."""
    argmax = probes(mi.NEVER)
    for s, g, k in SWITCHES[:3]:
        ref = mi.probe(s, g, switch_at=k)[1]
        assert ref["off_line"] and min(ref["off_line"]) <= k and set(range(k, len(ref["actions"]))) <= set(ref["off_line"]), (s, g, k)
        assert not any(ref["followed"]) and ref["actions"] == argmax[(s, g)]["actions"]
        assert ref["best"]["score"] > ref["score"]
    s, g, k = SWITCHES[3]
    ref = mi.probe(s, g, switch_at=k)[1]
    assert ref["followed"] == [mv >= k for mv in range(len(ref["actions"]))] and not ref["off_line"]
    assert ref["best"]["actions"] == ref["actions"]


@pytest.mark.parametrize("policy,land_pow", [(mi.UNIFORM, 0), (mi.WIDTH2, 2)])
def test_playout_incumbents_are_followed_past_the_tree(policy, land_pow):
    """Rollout evaluator, 3 playouts, the two smallest shapes: an incumbent that is a playout is followed past its tree_moves -- along
    the playout's own moves, which the search may never have tried (a followed action with zero visits)."""
    past = zero_visits = 0
    for s in (1, 4):
        for g in range(br.SHAPES[s][5]):
            ref = mi.probe(s, g, playouts=3, policy=policy, land_pow=land_pow)[1]
            mi.check_invariant(ref)
            for mv, (f, inc, counts) in enumerate(zip(ref["followed"], ref["running"], ref["fallback_counts"])):
                if f:
                    past += inc["playout"] >= 0 and mv >= inc["tree_moves"]
                    zero_visits += int(counts[ref["actions"][mv]]) == 0
    assert past >= 1 and zero_visits >= 1
