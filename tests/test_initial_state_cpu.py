"""Episodes from any state, the parts that need no GPU: the C ABI's new entry point in header and ctypes table, the reference
restatement (tests/initial_ref.py) pinned to the oracle's own episode loop, solve.Packing's initial board / present items and the
argument handling of solve.pack() / random_scores()."""
import os
import re

import numpy as np
import pytest

import evaluators as ev
import initial_ref as ir
import oracle_lib as orc
import rollout_ref as rr
from resource_packing_self_play_amd import _lib, solve
from resource_packing_self_play_amd.solve import Packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SALT = 9


def test_header_and_ctypes_table_declare_the_entry_point():
    text = open(os.path.join(ROOT, "include", "rp_engine.h")).read()
    assert re.search(r"\bint rp_set_instance_initial\(rp_ctx \*ctx, int64_t n, const uint64_t \*rows", text)
    assert int(re.search(r"#define RP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 9
    assert "rp_set_instance_initial" in _lib._SIGS and len(_lib._SIGS["rp_set_instance_initial"][1]) == 5
    assert callable(_lib.Engine.set_instance_initial)


@pytest.mark.parametrize("policy", [ir.ARGMAX_FIRST, ir.SAMPLE])
def test_play_from_the_empty_bin_is_the_oracles_episode(policy):
    W, H, N, _ = rr.GEOMETRIES["10x10/8"]
    rng = np.random.default_rng(5)
    buf = rr.BUFFERS["mixed"]
    for episode in range(3):
        wh, area = rr.make_items("10x10/8", rng)
        results = []
        for restated in (False, True):
            m = orc.OracleMCTS(W, H, N, 1.0, rr.ALPHA, lambda b, r: ev.table_eval("hashed", ev.pack_board(b), r, W * N, SALT),
                               lambda b, r: ev.tie_value(ev.pack_board(b), r, SALT))
            if restated:
                ir.begin(m, wh, np.ones(N, np.uint8), area, buf, SALT)
                got = ir.play_from(m, np.zeros((H, W), np.uint8), np.ones(N, np.uint8), 20, policy, 77, episode)
                results.append((got["actions"].tolist(), got["outcome"], got["score"], m.dump()))
            else:
                m.begin_episode(wh[:, 0], wh[:, 1], area, buf)
                actions, _, outcome, score = m.play_episode(20, policy=policy, seed=77, episode_id=episode, want_counts=False)
                results.append((actions.tolist(), outcome, score, m.dump()))
            m.close()
        assert results[0][:3] == results[1][:3] and len(results[0][0]) > 0
        assert results[0][3].keys() == results[1][3].keys()  # the same states were searched


def test_play_from_a_dead_state_is_an_episode_of_no_moves():
    W, H, N, _ = rr.GEOMETRIES["10x10/8"]
    wh = np.full((N, 2), 2, np.uint8)
    m = orc.OracleMCTS(W, H, N, 1.0, rr.ALPHA, lambda b, r: ev.table_eval("uniform", ev.pack_board(b), r, W * N, SALT), None)
    full = np.ones((H, W), np.uint8)
    ir.begin(m, wh, np.ones(N, np.uint8), W * H, [], SALT)
    got = ir.play_from(m, full, np.ones(N, np.uint8), 8, ir.ARGMAX_FIRST, 0, 0)
    assert (got["moves"], got["outcome"], got["score"]) == (0, 1, 1.0) and np.array_equal(got["board"], ev.pack_board(full))
    ir.begin(m, wh, np.zeros(N, np.uint8), 0, [0.5, 0.5], SALT)  # nobody takes part: max_h 0, cells == area == 0 -> r = 0 / 1
    got = ir.play_from(m, np.zeros((H, W), np.uint8), np.zeros(N, np.uint8), 8, ir.SAMPLE, 0, 0)
    assert (got["moves"], got["outcome"], got["score"]) == (0, -1, 0.0)
    m.close()


# ---- Packing ------------------------------------------------------------------------------------------------------------------
W6, H4 = 6, 4
WH = np.array([[2, 2], [2, 1], [2, 3]], np.uint8)
INITIAL = np.array([0b000011, 0b000001, 0, 0], np.uint64)  # cells (0, 0), (0, 1), (1, 0)


def fixed_packing(**kw):
    """Item 1 (2x1) at column 2 row 0, item 2 (2x3) at column 4 rows 0-2, on INITIAL; item 0 does not take part."""
    actions, masks = [1 * W6 + 2, 2 * W6 + 4], [0b1, 0b111]
    board = np.array([0b111111, 0b110001, 0b110000, 0], np.uint64)
    args = dict(initial_board=INITIAL, present=[0, 1, 1])
    args.update(kw)
    return Packing(3, W6, WH, args.pop("actions", actions), args.pop("masks", masks), args.pop("board", board), 1, 0.75, **args)


def test_packing_with_an_initial_board_and_absent_items():
    p = fixed_packing()
    assert np.array_equal(p.board_after(-1), INITIAL)
    assert np.array_equal(p.board_after(0), INITIAL | np.array([0b001100, 0, 0, 0], np.uint64))
    assert np.array_equal(p.board_after(1), p.board)
    lay = p.layout()
    assert lay.dtype == np.int8
    assert lay.tolist() == [[-2, -2, 1, 1, 2, 2], [-2, -1, -1, -1, 2, 2], [-1, -1, -1, -1, 2, 2], [-1] * 6]
    text = str(p).splitlines()
    assert "2 of 2 items placed" in text[0] and text[-2] == "  0 |##1122|" and text[-3] == "  1 |#...22|"
    assert p == fixed_packing() and p != fixed_packing(present=[1, 1, 1]) and p != fixed_packing(initial_board=None, board=p.board & ~INITIAL)


def test_packing_refuses_moves_over_fixed_cells_and_boards_without_them():
    with pytest.raises(ValueError, match="initially set"):
        fixed_packing(actions=[1 * W6 + 1, 2 * W6 + 4]).layout()  # item 1 at column 1 of row 0: cell (0, 1) is fixed
    with pytest.raises(ValueError, match="final board"):
        fixed_packing(board=np.array([0b111100, 0b110000, 0b110000, 0], np.uint64)).layout()  # the final bin lost the fixed cells
    with pytest.raises(ValueError, match="take part"):
        fixed_packing(actions=[0 * W6 + 2, 2 * W6 + 4])  # item 0 is absent
    with pytest.raises(ValueError):
        fixed_packing(initial_board=np.zeros(H4 + 1, np.uint64))
    with pytest.raises(ValueError):
        fixed_packing(present=[1, 1])


def test_packing_defaults_reproduce_the_views_without_the_new_fields():
    rng = np.random.default_rng(11)
    W, H, N = 8, 5, 10
    for _ in range(20):
        wh = np.stack([rng.integers(1, W // 2 + 2, N), rng.integers(1, H + 1, N)], axis=1).astype(np.uint8)
        board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
        actions, masks = [], []
        while True:
            valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
            if n == 0:
                break
            a = int(rng.choice(np.flatnonzero(valid)))
            _, nb, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, a)
            masks.append(sum(1 << int(r) for r in np.flatnonzero((nb != board).any(axis=1)))); actions.append(a); board = nb
        plain = Packing(4, W, wh, actions, masks, ev.pack_board(board), -1, 0.25)
        explicit = Packing(4, W, wh, actions, masks, ev.pack_board(board), -1, 0.25, initial_board=np.zeros(H, np.uint64), present=np.ones(N, bool))
        assert plain == explicit and str(plain) == str(explicit) and np.array_equal(plain.layout(), explicit.layout())
        assert (plain.layout() >= -1).all() and "%d of %d items placed" % (len(actions), N) in str(plain)
        assert not plain.initial_board.any() and plain.present.all()
        assert np.array_equal(plain.board_after(-1), np.zeros(H, np.uint64))


# ---- pack() / random_scores() arguments -------------------------------------------------------------------------------------------
def test_ragged_items_are_padded_with_items_that_do_not_take_part():
    W, H, N = 10, 10, 8
    ragged = [np.array([[3, 2], [4, 4]], np.uint8), np.array([[1, 1]] * 8, np.uint8), np.zeros((0, 2), np.uint8)]
    wh, rows, rem, area = solve.initial_state(W, H, N, ragged)
    assert wh.shape == (3, N, 2) and wh.dtype == np.uint8 and (wh >= 1).all()  # the padding is a legal item size for the pool
    assert rem.tolist() == [[1, 1] + [0] * 6, [1] * 8, [0] * 8] and not rows.any() and rows.shape == (3, H)
    assert wh[0, :2].tolist() == [[3, 2], [4, 4]] and area.tolist() == [22, 8, 0]
    with pytest.raises(ValueError, match="9 items"):
        solve.initial_state(W, H, N, [np.ones((9, 2), np.uint8)])


def test_default_total_area_counts_set_cells_and_present_items():
    W, H, N = 10, 10, 8
    full = np.full((2, N, 2), 2, np.uint8)
    assert solve.initial_state(W, H, N, full)[1:3] == (None, None)  # nothing new asked for: the pool starts as always
    cells = np.zeros((2, H, W), bool); cells[0, 0, :3] = True; cells[1, 2, 9] = True; cells[1, 0, 0] = True
    remaining = np.ones((2, N), np.uint8); remaining[1, 3:] = 0
    wh, rows, rem, area = solve.initial_state(W, H, N, full, cells, remaining)
    assert area.tolist() == [3 + 8 * 4, 2 + 3 * 4] and area.dtype == np.int32
    assert rows[0].tolist() == [0b111] + [0] * 9 and rows[1].tolist() == [1, 0, 1 << 9] + [0] * 7 and rows.dtype == np.uint64
    assert np.array_equal(rem, remaining)
    as_rows = solve.initial_state(W, H, N, full, rows, remaining)
    assert np.array_equal(as_rows[1], rows) and np.array_equal(as_rows[3], area)
    with pytest.raises(ValueError):
        solve.initial_state(W, H, N, full, cells[:, :5], remaining)
    with pytest.raises(ValueError):
        solve.initial_state(W, H, N, full, None, remaining[:, :4])


def test_seeds_with_an_initial_state_are_refused_before_any_engine_is_built():
    class Game:
        bin_width, bin_height, num_items = 10, 10, 8
    board = np.zeros((2, 10), np.uint64)
    for call in (lambda **kw: solve.pack(Game, None, None, seeds=[1, 2], **kw), lambda **kw: solve.random_scores(Game, seeds=[1, 2], **kw),
                 lambda **kw: solve.play_packings(None, seeds=[1, 2], **kw)):
        with pytest.raises(ValueError, match="seeds"):
            call(initial_board=board)
        with pytest.raises(ValueError, match="seeds"):
            call(remaining=np.ones((2, 8), np.uint8))
