"""CPU side of the playouts' landing power (rp_set_playout_landing): the C ABI's declarations, the Python surface, the restatement the
GPU tests hold the kernels to (tests/playout_landing_ref.py) against playout_policy_ref where the power is 0 and against the rule's own
definition where it is not, and the proof that the GPU test's inputs reach what they are there for."""
import os
import re

import numpy as np
import pytest

import playout_landing_ref as pl
import playout_policy_ref as pp
import rollout_prior_ref as rp
import rollout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SALT = pl.GPU_SEED, pl.GPU_SALT


def test_header_and_ctypes_table_have_the_entry_points():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("rp_set_playout_landing", 2), ("rp_playout_landing", 2)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "%s is not declared in include/rp_engine.h" % name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 10  # additive: the number stays
    version = text[text.index("#define RP_ABI_VERSION"):text.index("typedef enum rp_status")]
    assert "rp_set_playout_landing" in version and "rp_playout_landing" in version
    at = text.index("int rp_set_playout_landing(")
    comment = text[text.rindex("/*", 0, at):at]
    for cite in ("MCTS_bpp.py:87", "BinPackingGame.py:78-92", "BinPackingLogic.py:66-68", "2^37", "re-capture after switching"):
        assert cite in comment, cite
    # the policy keeps its two powers: the landing power is a setting of its own
    assert len(_lib._SIGS["rp_set_playout_policy"][1]) == 3 and _lib.PLAYOUT_POLICIES == pp.NAMES
    for method in ("set_playout_landing", "playout_landing"):
        assert callable(getattr(_lib.Engine, method))


def test_landing_power_accepts_and_rejects():
    from resource_packing_self_play_amd import _lib
    for x in (0, 1, 2, np.int32(2), np.uint8(1)):
        got = _lib.playout_landing_power(x)
        assert got == int(x) and type(got) is int
    assert _lib.playout_landing_power(None) == 0
    for bad in (-1, 3, 4, True, False, 1.0, 2.5, "1", "low", (1,), [2], np.float32(1)):
        with pytest.raises(ValueError):
            _lib.playout_landing_power(bad)


@pytest.mark.parametrize("name", list(rr.GEOMETRIES))
def test_power_zero_is_playout_policy_ref_step_for_step(name):
    W, H, N, _ = rr.GEOMETRIES[name]
    for wh, area, board, rem, eid in pp.gpu_states(name)[:1 if N == 128 else 3]:
        for policy in ((0, 0), (2, 0), (1, 1)):
            want, got = [], []
            a = pp.playout_path(W, H, N, board, rem, wh, SEED, eid, 1, trace=want, policy=policy)
            b = pl.playout_path(W, H, N, board, rem, wh, SEED, eid, 1, trace=got, policy=policy, land_pow=0)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert len(want) == len(got)
            for s, t in zip(want, got):
                assert np.array_equal(s[0], t[0]) and s[1:4] == t[1:4]
                assert all(s[4][k] == t[4][k] for k in ("T", "pick", "item", "bit", "c", "wt", "last"))
                assert t[4]["R"] == t[4]["c"] and t[4]["q"] == t[4]["bit"]  # L = 1
        assert pp.playout(W, H, N, board, rem, wh, area, rr.BUFFERS["mixed"], SEED, SALT, eid, 0, policy=(2, 0))[:3] == \
            pl.playout(W, H, N, board, rem, wh, area, rr.BUFFERS["mixed"], SEED, SALT, eid, 0, policy=(2, 0), land_pow=0)[:3]


def test_landing_rows_is_landing_row_of_every_column():
    rng = np.random.default_rng(3)
    for H, W in ((4, 4), (6, 40), (12, 12), (64, 64)):
        for fill in (0.1, 0.5, 0.9):
            board = (rng.random((H, W)) < fill).astype(np.uint8)
            for w in (1, 2, 3, W // 2, W):
                assert [int(t) for t in pl.landing_rows(board, w)] == [rp.landing_row(board, c, w) for c in range(W)]


def test_steps_keep_the_rule():
    """Every traced step from the definition: each move owns wt_i * L(i, c) consecutive units of [0, T) in ascending action order."""
    name = "20x20/32"
    W, H, N, _ = rr.GEOMETRIES[name]
    wh, area, board, rem, eid = pp.gpu_states(name)[1]
    for policy, land_pow in pl.GPU_SETTINGS:
        wt = pp.weights(wh, policy)
        trace = []
        moves, fb, fr = pl.playout_path(W, H, N, board, rem, wh, SEED, eid, 1, trace=trace, policy=policy, land_pow=land_pow)
        assert moves == len(trace)
        for mask, nv, x, a, s, b in trace:
            legal = np.flatnonzero(mask)
            own = [wt[k // W] * (H - rp.landing_row(b, int(k % W), int(wh[k // W, 0]))) ** land_pow for k in legal]
            assert sum(own) == s["T"] <= 1 << 37 and s["pick"] == rr.umulhi(x, s["T"])
            assert a == int(legal[np.searchsorted(np.cumsum(own), s["pick"], side="right")])
            assert s["q"] < s["R"] <= 1 << 18


def test_gpu_inputs_reach_what_they_are_for():
    """The states and settings of tests/test_gpu_playout_landing.py, from the restatement's traces."""
    seen = dict.fromkeys(("item >= 64", "T >= 2^32", "column neither first nor last", "q in the last column's span",
                          "item with two landing rows", "no-empty-row move legal", "exactly one legal move", "dead end with items left"), 0)
    differs = {}
    for name in pl.GEOMETRIES:
        W, H, N, _ = pl.GEOMETRIES[name]
        ref = pl.reference(name)
        for b, (wh, area, board, rem, eid) in enumerate(pl.gpu_states(name)):
            for setting in pl.gpu_settings(name, b):
                for j in range(pl.GPU_PLAYOUTS):
                    moves, fb, fr, acts, trace = ref[(setting, b, j)]
                    for mask, nv, x, a, s, bd in trace:
                        seen["item >= 64"] += s["item"] >= 64
                        seen["T >= 2^32"] += s["T"] >= 1 << 32
                        seen["column neither first nor last"] += 0 < s["bit"] < s["c"] - 1
                        seen["q in the last column's span"] += s["in_last_span"]
                        seen["item with two landing rows"] += len(set(s["rows"])) >= 2
                        seen["exactly one legal move"] += nv == 1
                        if name == "4x4/2":  # state A is there for it
                            for k in np.flatnonzero(mask):
                                seen["no-empty-row move legal"] += not rp.has_empty_row(bd, int(k % W), int(wh[k // W, 0]))
                    seen["dead end with items left"] += moves > 0 and int(fr.sum()) > 0
                    zero = []
                    pl.playout_path(W, H, N, board, rem, wh, SEED, eid, j, trace=zero, policy=setting[0], land_pow=0)
                    differs[name] = differs.get(name, 0) + ([t[3] for t in zero] != acts)
    assert all(seen.values()), seen
    assert all(differs[name] for name in pl.GEOMETRIES), differs  # a kernel that ignores the setting cannot pass on any geometry
