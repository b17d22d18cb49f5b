"""solve.Packing's derived views against the CPU oracle's rules (no GPU): random games driven with oracle_lib.valid_moves /
next_state, the (action, rows) trace read off consecutive boards exactly as the engine reads it off consecutive root keys."""
import os

import numpy as np
import pytest

import evaluators as ev
import oracle_lib as orc
from resource_packing_self_play_amd.solve import Packing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_shapes():
    g = np.load(os.path.join(GOLDEN, "game_rules.npz"))
    return sorted({(int(w), int(h), int(n)) for w, h, n in zip(g["W"], g["H"], g["N"])})


def guillotine(rng, W, H, N):
    items = [(W, H)]
    while len(items) < N:
        k = int(rng.integers(len(items))); w, h = items[k]
        if rng.integers(2) == 0:
            if w == 1: continue
            c = int(rng.integers(1, w)); items.pop(k); items += [(c, h), (w - c, h)]
        else:
            if h == 1: continue
            c = int(rng.integers(1, h)); items.pop(k); items += [(w, c), (w, h - c)]
    return np.array(items, np.uint8)


def random_game(rng, W, H, N, wh):
    """-> (boards after every move [(H, W) uint8], actions, rows masks) of one game of uniformly random legal moves."""
    board = np.zeros((H, W), np.uint8); rem = np.ones(N, np.uint8)
    boards, actions, masks = [], [], []
    while True:
        valid, n = orc.valid_moves(W, H, N, board, wh[:, 0], wh[:, 1], rem)
        if n == 0:
            return boards, actions, masks
        a = int(rng.choice(np.flatnonzero(valid)))
        rc, nb, rem = orc.next_state(W, H, N, board, wh[:, 0], wh[:, 1], rem, a)
        assert rc == 0
        changed = np.flatnonzero(ev.pack_board(nb) != ev.pack_board(board))  # rows where the key differs
        masks.append(sum(1 << int(r) for r in changed)); actions.append(a); boards.append(nb)
        board = nb


def minimal_bin_height(board):
    used = np.flatnonzero(board.sum(axis=1))
    return int(used[-1]) + 1 if len(used) else 1


def check_game(W, H, N, wh, boards, actions, masks, counts):
    final = ev.pack_board(boards[-1]) if boards else np.zeros(H, np.uint64)
    p = Packing(7, W, wh, actions, np.array(masks, np.uint64), final, 1, 0.5)
    assert p.moves == len(actions) and p.H == H and p.N == N
    assert np.array_equal(p.board_after(-1), np.zeros(H, np.uint64))
    placed = np.full((H, W), -1, np.int64)
    for m, a in enumerate(actions):
        assert (p.item[m], p.x[m]) == (a // W, a % W)
        assert np.array_equal(p.board_after(m), ev.pack_board(boards[m])), (W, H, N, m)
        rows = [r for r in range(H) if masks[m] >> r & 1]
        w, h = int(wh[a // W, 0]), int(wh[a // W, 1])
        run = not rows or rows == list(range(rows[0], rows[0] + len(rows)))  # no row at all: the item was discarded
        assert bool(p.contiguous[m]) == run and int(p.y[m]) == (rows[0] if rows else -1) and int(p.n_rows[m]) == len(rows)
        assert bool(p.partial[m]) == (len(rows) < h) and len(rows) <= h
        counts["moves"] += 1; counts["non_contiguous"] += not run; counts["partial"] += len(rows) < h; counts["discarded"] += not rows
        for r in rows:
            placed[r, a % W:a % W + w] = a // W
    lay = p.layout()
    assert lay.dtype == np.int8 and np.array_equal(lay, placed)
    assert np.array_equal(lay >= 0, (boards[-1] if boards else np.zeros((H, W))) > 0)  # occupied set == the final board, so no overlap either
    assert p.height == minimal_bin_height(boards[-1] if boards else np.zeros((H, W)))
    text = str(p)
    assert len(text.splitlines()) == H + 2 and "height %d" % p.height in text
    return p


# guillotine cuts of the whole bin (every item fits somewhere at first); then items far too large for the bin, so that the strip runs
# out under them (fewer than h rows) and free segments are separated by filled ones (non-contiguous rows)
CROWDED = [(6, 6, 8), (8, 5, 10), (40, 6, 9)]


def test_views_match_the_oracle_on_random_games():
    counts = dict(moves=0, non_contiguous=0, partial=0, discarded=0)
    shapes = golden_shapes()
    assert any(W > 32 for W, _, _ in shapes + CROWDED)
    rng = np.random.default_rng(2024)
    for (W, H, N) in shapes:
        for _ in range(2 if W * N > 2000 else 6):
            wh = guillotine(rng, W, H, N)
            check_game(W, H, N, wh, *random_game(rng, W, H, N, wh), counts)
    before = dict(counts)
    for (W, H, N) in CROWDED:
        for _ in range(40):
            wh = np.stack([rng.integers(1, W // 2 + 2, N), rng.integers(1, H + 1, N)], axis=1).astype(np.uint8)
            check_game(W, H, N, wh, *random_game(rng, W, H, N, wh), counts)
    print("moves %(moves)d, non-contiguous %(non_contiguous)d, cut short %(partial)d of which discarded %(discarded)d" % counts)
    # both classes are hit, by the golden shapes and by the crowded ones
    assert before["non_contiguous"] >= 10 and before["partial"] >= 10
    assert counts["non_contiguous"] > before["non_contiguous"] and counts["partial"] - before["partial"] >= 10 and counts["discarded"] >= 1
    assert counts["moves"] > 1000


def test_overlapping_or_incomplete_traces_make_layout_raise():
    W, H, N = 6, 4, 3
    wh = np.array([[2, 2], [2, 1], [2, 3]], np.uint8)
    # item 0 at column 0 rows 0-1, item 1 at column 2 row 0, item 2 at column 4 rows 0-2
    actions, masks = [0 * W + 0, 1 * W + 2, 2 * W + 4], [0b11, 0b1, 0b111]
    board = np.array([0b111111, 0b110011, 0b110000, 0], np.uint64)
    good = Packing(0, W, wh, actions, masks, board)
    assert good.layout()[0].tolist() == [0, 0, 1, 1, 2, 2] and good.height == 3 and good.contiguous.all() and not good.partial.any()
    overlapping = Packing(0, W, wh, [0 * W + 0, 1 * W + 1, 2 * W + 4], masks, board)  # item 1 moved onto item 0's cell (0, 1)
    with pytest.raises(ValueError, match="overlaps"):
        overlapping.layout()
    with pytest.raises(ValueError, match="final board"):
        Packing(0, W, wh, actions[:2], masks[:2], board).layout()  # the board holds an item the trace does not
    with pytest.raises(ValueError, match="leaves"):
        Packing(0, W, wh, [1 * W + 5], [0b1], board).layout()  # 2 wide at column 5 of 6
    with pytest.raises(ValueError):
        Packing(0, W, wh, [N * W], [1], board)  # action outside the action space
    split = Packing(0, W, wh, [2 * W + 0], [0b1011], np.array([0b11, 0b11, 0, 0b11], np.uint64))
    assert not split.contiguous[0] and split.y[0] == 0 and split.n_rows[0] == 3 and split.height == 4
    assert good == Packing(0, W, wh, actions, masks, board) and good != split
