"""CPU side of the playout policy (rp_set_playout_policy): the C ABI's declarations, the restatement the GPU tests hold the kernels to
(tests/playout_policy_ref.py) against rollout_ref and against its own probabilities, the proof that the GPU test's inputs reach every
branch of the weighted pick, and the probe of what the policies do to a playout -- pinned here and recorded in
profiles/playout_policy.md (run this file as a script to print the table)."""
import functools
import math
import os
import re

import numpy as np
import pytest

import evaluators as ev
import oracle_lib as orc
import playout_policy_ref as pp
import rollout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SALT = 20251, 77


def test_header_and_ctypes_table_have_the_entry_points():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("rp_set_playout_policy", 3), ("rp_playout_policy", 3)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "%s is not declared in include/rp_engine.h" % name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 10  # additive: the number stays
    at = text.index("int rp_set_playout_policy(")
    comment = text[text.rindex("/*", 0, at):at]
    for cite in ("MCTS_bpp.py:87", "BinPackingGame.py:78-92", "2^25"):
        assert cite in comment, cite
    assert _lib.PLAYOUT_POLICIES == pp.NAMES
    for method in ("set_playout_policy", "playout_policy"):
        assert callable(getattr(_lib.Engine, method))


def test_policy_names_and_pairs():
    from resource_packing_self_play_amd import _lib
    for name, pair in pp.NAMES.items():
        assert _lib.playout_policy_powers(name) == pair == _lib.playout_policy_powers(pair)
    assert _lib.playout_policy_powers(None) == (0, 0) and _lib.playout_policy_powers([1, 1]) == (1, 1)
    for bad in ("depth", "", (3, 0), (2, 1), (-1, 0), (1,), (1, 1, 0), 2, (1.0, 1.0), (True, 0)):
        with pytest.raises(ValueError):
            _lib.playout_policy_powers(bad)


@pytest.mark.parametrize("name", list(rr.GEOMETRIES))
def test_uniform_policy_is_rollout_ref_step_for_step(name):
    W, H, N, _ = rr.GEOMETRIES[name]
    for wh, area, board, rem, eid in pp.gpu_states(name)[:1 if N == 128 else 3]:
        for j in range(1 if N == 128 else 3):
            want, got = [], []
            a = rr.playout_path(W, H, N, board, rem, wh, SEED, eid, j, trace=want)
            b = pp.playout_path(W, H, N, board, rem, wh, SEED, eid, j, trace=got, policy=(0, 0))
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert len(want) == len(got)
            for s, t in zip(want, got):
                assert np.array_equal(s[0], t[0]) and s[1:] == t[1:4]
                assert t[4]["T"] == s[1] and t[4]["wt"] == 1  # T = nv, the pick is the uniform one
            if j == 0:
                assert rr.playout(W, H, N, board, rem, wh, area, rr.BUFFERS["mixed"], SEED, SALT, eid, j)[:3] == \
                    pp.playout(W, H, N, board, rem, wh, area, rr.BUFFERS["mixed"], SEED, SALT, eid, j)[:3]


def test_weighted_steps_keep_the_rule():
    """Every traced step of a weighted playout, from the definitions: the pick's unit lies inside the chosen move's wt units."""
    name = "20x20/32"
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, board, rem, eid = pp.gpu_states(name)[1]
    for policy in pp.NAMES.values():
        wt = pp.weights(wh, policy)
        trace = []
        moves, fb, fr = pp.playout_path(W, H, N, board, rem, wh, SEED, eid, 1, trace=trace, policy=policy)
        assert moves == len(trace) and orc.valid_moves(W, H, N, fb, wh[:, 0], wh[:, 1], fr)[1] == 0
        for mask, nv, x, a, s in trace:
            legal = np.flatnonzero(mask)
            units = np.repeat(legal, [wt[k // W] for k in legal])  # the moves in ascending action order, wt units each
            assert len(units) == s["T"] and s["pick"] == rr.umulhi(x, s["T"]) and a == int(units[s["pick"]])
            assert 1 <= s["wt"] <= 4096 and s["T"] <= 1 << 25


def test_step_frequencies_follow_the_weights():
    """4096 playout indices at step 0 of one fixed state: the frequency f of every item lies within 5 sqrt(p (1 - p) / n) of
    p = c_i wt_i / T."""
    name, n = "20x20/32", 4096
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, board, rem, eid = pp.gpu_states(name)[1]
    mask, nv = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
    c = (mask.reshape(N, W) != 0).sum(axis=1)
    h0 = ev.splitmix64(ev.key_hash(ev.pack_board(board), rem, SEED) ^ eid)
    draws = [orc.lib().orc_sample_u64(h0, j, 0) for j in range(n)]
    for policy in ((1, 1), (2, 0), (0, 2)):
        wt = pp.weights(wh, policy)
        assert len({wt[i] for i in range(N) if c[i]}) >= 3, "the state needs three legal items of different weights"
        T = sum(int(c[i]) * wt[i] for i in range(N))
        hits = np.zeros(N, np.int64)
        for x in draws:
            a, s = pp.pick_move(mask, W, N, wt, x)
            assert mask[a] and a // W == s["item"]
            hits[s["item"]] += 1
        for i in range(N):
            p = int(c[i]) * wt[i] / T
            assert abs(hits[i] / n - p) <= 5 * math.sqrt(p * (1 - p) / n), (policy, i, hits[i] / n, p)


def test_gpu_inputs_reach_every_branch_of_the_pick():
    """The states, instances and policies of tests/test_gpu_playout_policy.py, from the restatement's trace."""
    seen = dict.fromkeys(("item >= 64", "not the first legal column", "weight >= 1024", "T >= 2^16", "pick in the last legal item",
                          "exactly one legal move", "dead end with items left"), 0)
    for name in rr.GEOMETRIES:
        W, H, N, _ = rr.GEOMETRIES[name]
        for wh, area, board, rem, eid in pp.gpu_states(name):
            for policy in pp.GPU_POLICIES:
                for j in range(pp.GPU_PLAYOUTS):
                    trace = []
                    moves, fb, fr = pp.playout_path(W, H, N, board, rem, wh, pp.GPU_SEED, eid, j, trace=trace, policy=policy)
                    for mask, nv, x, a, s in trace:
                        seen["item >= 64"] += s["item"] >= 64
                        seen["not the first legal column"] += s["bit"] > 0
                        seen["weight >= 1024"] += s["wt"] >= 1024
                        seen["T >= 2^16"] += s["T"] >= 1 << 16
                        seen["pick in the last legal item"] += s["last"]
                        seen["exactly one legal move"] += nv == 1
                    seen["dead end with items left"] += moves > 0 and int(fr.sum()) > 0
    assert all(seen.values()), seen


# ---- the probe: what a policy does to the playouts ------------------------------------------------------------------------------------------
# board W x H, N items cut from W x bin_h; 12 instances of rollout_ref.cut_items (generator seed 2025), 24 playouts each from the empty
# bin, engine seed 5, empty buffer.  The score is r of BinPackingGame.py:188-212; a dead end (items left over) scores 0.
PROBE_SHAPES = ((20, 20, 12, 32), (20, 20, 15, 32), (20, 20, 15, 16), (10, 10, 7, 8))
PROBE_INSTANCES, PROBE_PLAYOUTS, PROBE_SEED, PROBE_GEN = 12, 24, 5, 2025
# (shape, policy) -> (mean r, dead ends of 288, mean of the per-instance best), the restatement's own figures to six places
PROBE_PINNED = {
    ((20, 20, 12, 32), 'uniform'): (0.312918, 155, 0.745717),
    ((20, 20, 12, 32), 'area'): (0.388663, 119, 0.737050),
    ((20, 20, 12, 32), 'width'): (0.467614, 83, 0.729752),
    ((20, 20, 12, 32), 'width2'): (0.524210, 57, 0.752069),
    ((20, 20, 12, 32), 'height'): (0.304208, 160, 0.741115),
    ((20, 20, 12, 32), 'height2'): (0.270336, 176, 0.710171),
    ((20, 20, 15, 32), 'uniform'): (0.082468, 257, 0.583763),
    ((20, 20, 15, 32), 'area'): (0.205674, 211, 0.795816),
    ((20, 20, 15, 32), 'width'): (0.207788, 210, 0.791000),
    ((20, 20, 15, 32), 'width2'): (0.326133, 165, 0.812199),
    ((20, 20, 15, 32), 'height'): (0.093996, 253, 0.663076),
    ((20, 20, 15, 32), 'height2'): (0.070967, 262, 0.464912),
    ((20, 20, 15, 16), 'uniform'): (0.105171, 250, 0.680373),
    ((20, 20, 15, 16), 'area'): (0.294502, 182, 0.859724),
    ((20, 20, 15, 16), 'width'): (0.194489, 218, 0.816037),
    ((20, 20, 15, 16), 'width2'): (0.387508, 148, 0.853721),
    ((20, 20, 15, 16), 'height'): (0.135431, 240, 0.711623),
    ((20, 20, 15, 16), 'height2'): (0.174428, 226, 0.786276),
    ((10, 10, 7, 8), 'uniform'): (0.414072, 134, 0.922917),
    ((10, 10, 7, 8), 'area'): (0.511111, 100, 0.958333),
    ((10, 10, 7, 8), 'width'): (0.483526, 107, 0.902778),
    ((10, 10, 7, 8), 'width2'): (0.616782, 59, 0.958333),
    ((10, 10, 7, 8), 'height'): (0.368297, 153, 0.918981),
    ((10, 10, 7, 8), 'height2'): (0.397184, 142, 0.893981),
}


@functools.lru_cache(maxsize=None)
def probe(shape):
    """-> {policy name: (mean r, dead ends, mean of the per-instance best)}"""
    W, H, bin_h, N = shape
    rng = np.random.default_rng(PROBE_GEN)
    insts = [rr.cut_items(rng, W, bin_h, N) for _ in range(PROBE_INSTANCES)]
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    out = {}
    for pname, policy in pp.NAMES.items():
        r = np.array([[pp.playout(W, H, N, board, rem, wh, W * bin_h, [], PROBE_SEED, 0, i, j, policy=policy)[1] for j in range(PROBE_PLAYOUTS)]
                      for i, wh in enumerate(insts)])
        out[pname] = (float(r.mean()), int((r == 0).sum()), float(r.max(axis=1).mean()))
    return out


def probe_row(shape, pname, fig):
    return "| %dx%d / %d (%dx%d) | %s | %.6f | %d | %.6f |" % (shape[0], shape[1], shape[3], shape[0], shape[2], pname, fig[0], fig[1], fig[2])


@pytest.mark.parametrize("shape", PROBE_SHAPES, ids=lambda s: "%dx%d/%d(%dx%d)" % (s[0], s[1], s[3], s[0], s[2]))
def test_probe_width2_beats_uniform_and_the_figures_are_pinned(shape):
    got = probe(shape)
    assert got["width2"][0] > got["uniform"][0] and got["width2"][1] < got["uniform"][1], got
    doc = open(os.path.join(ROOT, "profiles", "playout_policy.md")).read()
    for pname, fig in got.items():
        want = PROBE_PINNED[(shape, pname)]
        assert fig[1] == want[1] and fig[0] == pytest.approx(want[0], abs=1e-6) and fig[2] == pytest.approx(want[2], abs=1e-6), (pname, fig, want)
        assert probe_row(shape, pname, want) in doc, "profiles/playout_policy.md does not carry the pinned row of %s" % pname


if __name__ == "__main__":
    for shape in PROBE_SHAPES:
        for pname, fig in probe(shape).items():
            print(probe_row(shape, pname, fig), "   # %r: (%.6f, %d, %.6f)," % ((shape, pname), fig[0], fig[1], fig[2]))
