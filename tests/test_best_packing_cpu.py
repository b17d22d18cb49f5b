"""CPU side of the incumbents (rp_set_incumbent): solve.replay_rows against the oracle's rules, the C ABI's declarations, and a guard
that the oracle-side reference of tests/test_gpu_best_packing.py is not vacuous on the shapes that test plays."""
import os
import re

import numpy as np
import pytest

import best_ref
import evaluators as ev
import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_sequence(rng, W, H, N, board, max_side):
    """A random legal sequence from `board` ([H, W] cells) to a state without a legal move -> (wh, actions, rows masks, final cells)."""
    wh = np.stack([rng.integers(1, max_side + 1, N), rng.integers(1, max_side + 1, N)], axis=1).astype(np.uint8)
    rem = np.ones(N, np.uint8)
    actions, rows = [], []
    while True:
        valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        if n == 0:
            return wh, actions, rows, board
        a = int(rng.choice(np.flatnonzero(valid)))
        rc, after, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, a)
        assert rc == 0
        rows.append(sum(1 << int(r) for r in np.flatnonzero((after != board).any(axis=1))))
        actions.append(a)
        board = after


@pytest.mark.parametrize("W,H,N,max_side,fill", [(10, 10, 8, 5, 0.0), (7, 9, 12, 4, 0.25), (32, 6, 10, 9, 0.2), (40, 6, 9, 12, 0.0), (64, 5, 8, 20, 0.3)])
def test_replay_rows_is_execute_move(W, H, N, max_side, fill):
    from resource_packing_self_play_amd.solve import Packing, replay_rows
    rng = np.random.default_rng(W * 1000 + H * 10 + N)
    seen = dict(cut=0, split=0, moves=0)
    for case in range(12):
        board = (rng.random((H, W)) < fill).astype(np.uint8)
        initial = ev.pack_board(board) if fill else None
        wh, actions, rows, final = random_sequence(rng, W, H, N, board, max_side)
        got_rows, got_board = replay_rows(W, H, wh, actions, initial)
        assert got_rows.dtype == np.uint64 and got_board.dtype == np.uint64 and got_board.shape == (H,)
        assert [int(r) for r in got_rows] == rows, (case, actions)
        assert np.array_equal(got_board, ev.pack_board(final))
        p = Packing(case, W, wh, actions, got_rows, got_board, initial_board=initial)
        p.layout()
        seen["cut"] += int(p.partial.sum()); seen["split"] += int((~p.contiguous).sum()); seen["moves"] += p.moves
    assert seen["moves"] > 0 and seen["cut"] > 0, "no move was cut short: the cases do not cover it"
    if fill:
        assert seen["split"] > 0, "no move landed in non-contiguous rows: the cases do not cover it"


def test_replay_rows_refuses_a_bad_action():
    from resource_packing_self_play_amd.solve import replay_rows
    with pytest.raises(ValueError):
        replay_rows(4, 4, [[1, 1]], [4])
    rows, board = replay_rows(4, 3, [[2, 2]], [])
    assert len(rows) == 0 and not board.any()


def test_header_and_bindings_declare_the_incumbent_abi():
    from resource_packing_self_play_amd import _lib
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == 10 == _lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rp_set_incumbent", "rp_pop_finished_best", "rp_incumbents"):
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, code)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]), name
    # the comments say what the reference does at that point, and what the feature costs
    for cite in ("MCTS_bpp.py:78-83", "BinPackingGame.py:188-212"):
        assert text.count(cite) >= 3, cite
    assert "(G + fin_cap) * S + 16 G bytes" in text
    for method in ("set_incumbent", "incumbents"):
        assert hasattr(_lib.Engine, method)


def test_reference_is_not_vacuous_on_the_probe_shapes():
    """Over the five shapes, with the sampled move rule: some episode's tree holds a terminal that scores strictly above the played
    packing, and in some episode several terminals share the maximum and the incumbent -- the first of them -- is not the last."""
    better = first_not_last = episodes = 0
    for W, H, bin_h, N, sims, games in best_ref.SHAPES:
        wh = best_ref.instances(W, bin_h, N, games)
        for g in range(games):
            _, _, score, ref = best_ref.oracle_episode(W, H, N, wh[g], W * bin_h, best_ref.BUF, best_ref.KINDS[g % 2], sims, best_ref.SAMPLE,
                                                       best_ref.SEED, g)
            assert ref["score"] >= score and 1 <= ref["updates"] <= ref["terminals"]
            better += ref["score"] > score
            first_not_last += ref["ties"] > 1 and ref["index"] != ref["last"]
            episodes += 1
    assert episodes == 32
    assert better >= 1, "no episode's tree beats its played packing: the GPU parity test would prove little"
    assert first_not_last >= 1, "the tie rule (first created among equals) is never exercised"
