"""CPU-side checks of the random-playout evaluator: the C ABI declares it and the ctypes table binds it, and the Python restatement
that the GPU tests hold the kernels to (tests/rollout_ref.py) keeps its own invariants on every geometry those tests use."""
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
import rollout_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SALT = 20251, 77


def test_header_and_ctypes_table_have_the_entry_points():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("rp_rollout_eval", 5), ("rp_rollout_states", 16)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "%s is not declared in include/rp_engine.h" % name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 8
    for name in ("rp_rollout_eval", "rp_rollout_states"):  # each comment cites the predict call the playouts stand in for
        at = text.index("int %s(" % name)
        assert "MCTS_bpp.py:87" in text[text.rindex("/*", 0, at):at], name


@pytest.mark.parametrize("name", list(ref.GEOMETRIES))
def test_restatement_invariants(name):
    W, H, N, _ = ref.GEOMETRIES[name]
    rng = np.random.default_rng(N * 131 + W)
    wh, area = ref.make_items(name, rng)
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    for j in range(1 if N == 128 else 2):
        trace = []
        moves, fb, fr = ref.playout_path(W, H, N, board, rem, wh, SEED, 5, j, trace)
        assert moves == len(trace) <= N
        assert orc.valid_moves(W, H, N, fb, wh[:, 0], wh[:, 1], fr)[1] == 0, "the playout stopped before the state was terminal"
        assert int(fr.sum()) == N - moves  # every move placed exactly one item
        for mask, nv, x, a in trace:
            assert nv == int(mask.sum()) > 0
            k = ref.umulhi(x, nv)
            assert 0 <= k < nv and a == int(np.flatnonzero(mask)[k])
        # the value a leaf gets is a mean of +-1 outcomes, whatever the buffer
        for buf in ref.BUFFERS.values():
            e, r = ref.rank(W, H, fb, fr, area, int(wh[:, 1].max()), buf, SALT)
            assert e in (1, -1) and 0.0 <= r <= 1.0
            if not buf:
                assert e == 1


def test_playouts_differ_by_index_and_episode_but_not_by_call():
    W, H, N, _ = ref.GEOMETRIES["10x10/8"]
    wh, area = ref.make_items("10x10/8", np.random.default_rng(3))
    board, rem = np.zeros((H, W), np.uint8), np.ones(N, np.uint8)
    runs = {(e, j): ref.playout(W, H, N, board, rem, wh, area, [], SEED, SALT, e, j) for e in (0, 1) for j in range(4)}
    again = ref.playout(W, H, N, board, rem, wh, area, [], SEED, SALT, 1, 2)
    assert again[:3] == runs[(1, 2)][:3] and np.array_equal(again[3], runs[(1, 2)][3])
    assert len({r[3].tobytes() for r in runs.values()}) > 1, "eight playouts, one packing: the draws do not depend on (episode, playout)"
    pi, v = ref.evaluator(W, H, N, wh, area, [], SEED, SALT, 0, 4)(board, rem)
    assert pi.dtype == np.float32 and v.dtype == np.float32 and v[0] == 1.0 and pi[0] == np.float32(1) / np.float32(W * N)
