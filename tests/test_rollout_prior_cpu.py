"""CPU side of the rollout prior (rp_set_rollout_prior): the C ABI's declarations, the restatement the GPU tests hold the kernel to
(tests/rollout_prior_ref.py) against the oracle's rules, and the proof that the GPU test's inputs reach what they are for -- the
fall-through of t, a 64-bit T, the candidate rule beyond 64 legal moves, and searches that the prior changes."""
import os
import re

import numpy as np
import pytest

import oracle_lib as orc
import rollout_prior_ref as rp
import rollout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_ctypes_table_have_the_entry_points():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("rp_set_rollout_prior", 4), ("rp_rollout_prior", 4), ("rp_rollout_prior_states", 6)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, "%s is not declared in include/rp_engine.h" % name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == n_args
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 10  # additive: the number stays
    at = text.index("int rp_set_rollout_prior(")
    comment = text[text.rindex("/*", 0, at):at]
    for cite in ("BinPackingGame.py:78-92", "BinPackingLogic.py:66-68", "BinPackingLogic.py:103-105", "BinPackingLogic.py:89", "MCTS_bpp.py:88-100", "2^37"):
        assert cite in comment, cite
    assert _lib.ROLLOUT_PRIORS == rp.NAMES
    for method in ("set_rollout_prior", "rollout_prior", "rollout_prior_states"):
        assert callable(getattr(_lib.Engine, method))


def test_the_rule_is_stated_in_the_same_words():
    """The header, DESIGN.md and README.md carry the rule of the restatement's docstring."""
    def words(s):
        return " ".join(s.replace("*", " ").replace("`", "").split())
    rule = rp.__doc__[rp.__doc__.index("  - For a leaf state"):]
    header = words(open(os.path.join(ROOT, "include", "rp_engine.h")).read())
    design = words(open(os.path.join(ROOT, "DESIGN.md")).read())
    for line in rule.strip().split("\n  - "):
        assert words(line.lstrip(" -")) in header, line
    for key in ("u(i, c) = w_i^w_pow * h_i^h_pow * (H - t(i, c))^land_pow", "pi[a] = float32(float64(u) / float64(T))", "2^37"):
        assert words(key) in design, key
        assert words(key) in words(open(os.path.join(ROOT, "README.md")).read()), key


def test_prior_names_and_triples():
    from resource_packing_self_play_amd import _lib
    for name, triple in rp.NAMES.items():
        assert _lib.rollout_prior_powers(name) == triple == _lib.rollout_prior_powers(triple)
    assert _lib.rollout_prior_powers(None) == (0, 0, 0) and _lib.rollout_prior_powers([1, 1, 2]) == (1, 1, 2)
    for bad in ("depth", "", (3, 0, 0), (2, 1, 0), (-1, 0, 0), (0, 0, 3), (0, 0, -1), (1, 1), (1, 1, 0, 0), 2, (1.0, 1.0, 0.0), (True, 0, 0)):
        with pytest.raises(ValueError):
            _lib.rollout_prior_powers(bad)


@pytest.mark.parametrize("name", list(rp.GEOMETRIES))
def test_landing_row_is_the_row_the_move_fills_first(name):
    """Every legal move of the chosen states whose window has an empty row: t is the lowest row next_state changes."""
    W, H, N, _ = rp.GEOMETRIES[name]
    checked = 0
    for wh, area, board, rem, eid in rp.gpu_states(name):
        mask, nv = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        legal = np.flatnonzero(mask)
        if N == 128:  # 8 192 actions: every 37th legal move
            legal = legal[::37]
        for a in legal:
            i, c = divmod(int(a), W)
            if not rp.has_empty_row(board, c, int(wh[i, 0])):
                continue
            rc, nb, _ = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, int(a))
            assert rc == 0
            changed = np.flatnonzero((np.asarray(nb).reshape(H, W) != board).any(axis=1))
            assert changed.size and int(changed[0]) == rp.landing_row(board, c, int(wh[i, 0])), (name, int(a))
            checked += 1
    assert checked


def test_state_a_has_a_legal_move_without_an_empty_row():
    wh, area, board, rem, eid = rp.state_a()
    mask, nv = orc.valid_moves(4, 4, 2, board, wh[:, 0], wh[:, 1], rem)
    assert nv == 4 and mask[0]
    assert not rp.has_empty_row(board, 0, 2) and rp.landing_row(board, 0, 2) == 3
    rc, nb, _ = orc.next_state(4, 4, 2, board, wh[:, 0], wh[:, 1], rem, 0)
    assert rc == 0 and np.array_equal(np.asarray(nb).reshape(4, 4), board)  # playing it changes no cell
    assert rp.weights(4, 4, 2, board, rem, wh, (0, 0, 2))[0] == 1


def test_state_b_needs_a_64_bit_sum():
    wh, area, board, rem, eid = rp.state_b()
    mask, nv = orc.valid_moves(64, 64, 128, board, wh[:, 0], wh[:, 1], rem)
    assert nv == 4096 and mask.reshape(128, 64)[:, 1::2].all() and not mask.reshape(128, 64)[:, 0::2].any()
    T = sum(rp.weights(64, 64, 128, board, rem, wh, rp.PRIOR_B))
    assert T == 2 ** 36 >= 2 ** 32
    assert rp.PRIOR_B in rp.gpu_priors("64x64/128", len(rp.gpu_states("64x64/128")) - 1)


def test_a_state_has_more_than_64_legal_moves_with_unequal_weights():
    """Beyond 64 legal moves the search keeps one candidate of all unvisited moves, the largest pi: it matters there."""
    found = []
    for name in rr.GEOMETRIES:
        W, H, N, _ = rr.GEOMETRIES[name]
        for k, (wh, area, board, rem, eid) in enumerate(rp.gpu_states(name)):
            u = [x for x in rp.weights(W, H, N, board, rem, wh, (2, 0, 2)) if x]
            if len(u) > 64 and len(set(u)) > 1:
                found.append((name, k))
    assert found
    wh, area, buf, eid = rp.search_instance("12x12/70")  # and at the root of the N > 64 search case
    u = [x for x in rp.weights(12, 12, 70, np.zeros((12, 12), np.uint8), np.ones(70, np.uint8), wh, rp.PRIOR_SEARCH) if x]
    assert len(u) >= 70 and len(set(u)) > 1


@pytest.mark.parametrize("name", list(rp.GEOMETRIES))
def test_rows_are_zero_at_the_illegal_actions_and_sum_to_one(name):
    W, H, N, _ = rp.GEOMETRIES[name]
    A = W * N
    for k, (wh, area, board, rem, eid) in enumerate(rp.gpu_states(name)):
        mask, nv = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        assert nv > 0
        for prior in rp.gpu_priors(name, k):
            row = rp.prior_row(W, H, N, board, rem, wh, prior)
            assert row.dtype == np.float32 and row.shape == (A,)
            assert np.array_equal(row != 0, np.asarray(mask) != 0)
            assert abs(float(row.astype(np.float64).sum()) - 1.0) <= A * 2.0 ** -24
        assert np.array_equal(rp.prior_row(W, H, N, board, rem, wh, (0, 0, 0)), np.full(A, np.float32(1) / np.float32(A), np.float32))
    # a state without a legal move: all zero
    assert not rp.prior_row(W, H, N, np.ones((H, W), np.uint8), np.ones(N, np.uint8), rp.gpu_states(name)[0][0], (2, 0, 2)).any()


@pytest.mark.parametrize("name", list(rp.SEARCH_CASES))
def test_the_prior_changes_the_search_cases(name):
    """The oracle's first root counts under the prior differ from those under the uniform prior: the GPU test cannot pass with the
    prior ignored."""
    assert not np.array_equal(rp.first_root_counts(name, rp.PRIOR_SEARCH), rp.first_root_counts(name, rp.UNIFORM))
