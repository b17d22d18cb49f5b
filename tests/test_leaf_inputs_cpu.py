"""The inputs and references of tests/test_gpu_leaf_inputs.py, checked on the host (tests/leaf_inputs_ref.py): the chosen states are
legal where they must be and reach the table entries and branches they were chosen for, and the float64 stem reference and the
header's accuracy bound are what they claim to be."""
import numpy as np
import pytest

import leaf_inputs_ref as ref
import oracle_lib as orc


@pytest.mark.parametrize("geometry", ref.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_states_have_a_legal_move_and_the_full_board_has_none(geometry):
    W, H, N = geometry
    st = ref.states(W, H, N)
    assert len(st) == ref.STATES_PER_GEOMETRY + (2 if geometry == ref.TILE_GEOMETRY else 0)
    full = ref.ev.unpack_board(ref.terminal_rows(W, H), W)
    assert full.all()
    for k in range(len(st)):
        iw, ih = st.wh[k, :, 0], st.wh[k, :, 1]
        assert st.rem[k, 0] == 1 and tuple(st.wh[k, 0]) == (1, 1) and not st.board(k)[:, 0].all()
        assert (iw >= 1).all() and (iw <= W).all() and (ih >= 1).all() and (ih <= H).all()
        assert int(st.rows[k].max()) >> W == 0
        assert orc.valid_moves(W, H, N, st.board(k), iw, ih, st.rem[k])[1] > 0, k
        assert orc.valid_moves(W, H, N, full, iw, ih, st.rem[k])[1] == 0, k


def test_every_grid_pattern_occurs_and_the_borders_see_cells():
    seen = np.zeros(512, bool)
    borders = {name: False for name in ("top", "bottom", "left", "right", "tl", "tr", "bl", "br")}
    for W, H, N in ref.GEOMETRIES:
        st = ref.states(W, H, N)
        for k in range(len(st)):
            pat = ref.grid_patterns(st.board(k))
            seen[np.unique(pat)] = True
            if W >= 3 and H >= 3:  # borders and corners that are distinct cells
                for name, part in (("top", pat[0, 1:-1]), ("bottom", pat[-1, 1:-1]), ("left", pat[1:-1, 0]), ("right", pat[1:-1, -1]),
                                   ("tl", pat[0, 0]), ("tr", pat[0, -1]), ("bl", pat[-1, 0]), ("br", pat[-1, -1])):
                    borders[name] = borders[name] or bool(np.any(part != 0))
    assert seen.all(), "grid patterns never indexed: %s" % np.nonzero(~seen)[0]
    assert all(borders.values()), borders
    tiles = ref.states(*ref.TILE_GEOMETRY)
    for half in range(2):  # the tile boards alone carry all 512, each at its tile's centre
        pat = ref.grid_patterns(tiles.board(ref.STATES_PER_GEOMETRY + half))
        assert np.array_equal(pat[1::4, 1::4].reshape(-1), 256 * half + np.arange(256))
        assert not tiles.board(ref.STATES_PER_GEOMETRY + half)[3::4].any() and not tiles.board(ref.STATES_PER_GEOMETRY + half)[:, 3::4].any()


def test_item_sizes_and_remaining_sets_cover_the_directed_cases():
    for W, H, N in ref.GEOMETRIES:
        st = ref.states(W, H, N)
        sizes = {tuple(x) for k in range(len(st)) for x in st.wh[k]}
        if N >= 3:
            assert {(1, 1), (W, H), (W, 1), (1, H)} <= sizes, (W, H, N)
        if N >= 32:  # room for all of them
            assert {(a, b) for a in (7, 8, 9) for b in (7, 8, 9) if a <= W and b <= H} <= sizes, (W, H, N)
        counts = st.rem.astype(bool).sum(axis=1)
        assert counts.max() == N and counts.min() == 1


def test_both_sides_of_the_corner_phase_threshold():
    held = 0
    for W, H, N in ref.GEOMETRIES:
        st = ref.states(W, H, N)
        small = [ref.small_items(st.rem[k], st.wh[k], W) for k in range(len(st))]
        if N >= ref.CORNER_MIN_ITEMS:  # every geometry that can reach the threshold has states on both sides, whatever its corner
            assert max(small) >= ref.CORNER_MIN_ITEMS and min(small) < ref.CORNER_MIN_ITEMS, (W, H, N, small)
        if N >= ref.CORNER_MIN_ITEMS and ref.corner_dims(W) == (8, 8):
            held += 1
            hs = {int(st.wh[k, i, 1]) for k in range(len(st)) for i in range(N) if st.rem[k, i]}
            ws = {int(st.wh[k, i, 0]) for k in range(len(st)) for i in range(N) if st.rem[k, i]}
            assert {7, 8} <= hs and {7, 8, 9} <= ws, (W, H, N)  # unplaced sizes around CR x CC (9 high does not fit H = 8, 9)
    assert held == 4  # 20x20/32, 32x9/40, 33x8/41, 12x64/65
    assert ref.corner_dims(2) == (8, 2) and ref.corner_dims(6) == (8, 6) and ref.corner_dims(64) == (4, 8) and ref.corner_dims(1) == (8, 2)


def test_launch_forms_of_the_geometries():
    assert ref.table_in_lds(40) and not ref.table_in_lds(41)
    assert [ref.table_in_lds(N) for _, _, N in ref.GEOMETRIES] == [True, True, True, True, True, False, True, False, False, False]
    assert ref.stem_passes(1, 1) == 1 and ref.stem_passes(20, 20) == 2 and ref.stem_passes(64, 1) == 1
    assert ref.stem_passes(64, 64) == 1 + -(-(32 * 32 - 64) // 31)  # at Wp = 32 a pass advances 31 pixels


def test_pipeline_slots_and_packed_sets():
    W, H, N = ref.PIPELINE_GEOMETRY
    st = ref.states(W, H, N, ref.PIPELINE_STATES)
    assert len({(st.rows[k].tobytes(), st.rem[k].tobytes(), st.wh[k].tobytes()) for k in range(len(st))}) == ref.PIPELINE_STATES
    for k in range(len(st)):
        assert orc.valid_moves(W, H, N, st.board(k), st.wh[k, :, 0], st.wh[k, :, 1], st.rem[k])[1] > 0
    games = 40 * 256 + 5
    order, terminal = ref.pipeline_slots(games)
    assert np.array_equal(np.bincount(order, minlength=64), np.bincount(np.arange(games) % 64)) and not np.array_equal(order, np.arange(games) % 64)
    assert terminal[6] and terminal.sum() == games // 7 and not terminal[:6].any()
    assert ref.persistent_trips(games, 256) == 4 and ref.persistent_trips(64, 256) == 1 and ref.persistent_trips(40 * 304 + 5, 304) == 4
    for W, H, N in ref.GEOMETRIES:
        d, E, A = ref.packed_set(W, H, N), len(ref.states(W, H, N)), W * N
        assert d["key"].shape == (E, ref.key_words(W, H, N)) and d["key"].dtype == np.uint32 and d["sp_off"].dtype == np.int64
        assert np.array_equal(d["sp_off"], np.cumsum(d["sp_n"]) - d["sp_n"]) and int(d["sp_n"].sum()) == len(d["sp_act"]) == len(d["sp_cnt"])
        assert d["sp_n"][1] == 0 and int(d["sp_act"].max()) < A and int(d["sp_cnt"].max()) == 2 ** 32 - 1 and int(d["sp_cnt"].min()) >= 1
        assert ref.key_words(W, H, N) % 2 == 0 or W <= 32
        pi = ref.expected_pi(d, A, 0)
        assert pi.dtype == np.float32 and abs(float(pi.astype(np.float64).sum()) - 1) < 1e-5 and not ref.expected_pi(d, A, 1).any()


def _brute_force_count(st, k):
    """All-ones channel: set taps of the 3x3 window over the grid plane and every unplaced item's rectangle, then the 3x3 / 2 pool."""
    W, H = st.W, st.H
    board, rem, w, h = st.board(k), st.rem[k].astype(bool), st.wh[k, :, 0].astype(int), st.wh[k, :, 1].astype(int)
    conv = np.zeros((H, W), np.int64)
    for r in range(H):
        for x in range(W):
            for dr in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    rr, xx = r + dr, x + dx
                    if 0 <= rr < H and 0 <= xx < W:
                        conv[r, x] += int(board[rr, xx]) + int((rem & (rr < h) & (xx < w)).sum())
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((Hp, Wp), np.int64)
    for pr in range(Hp):
        for px in range(Wp):
            out[pr, px] = max(conv[r, x] for r in range(max(0, 2 * pr - 1), min(H, 2 * pr + 2)) for x in range(max(0, 2 * px - 1), min(W, 2 * px + 2)))
    return out


@pytest.mark.parametrize("geometry", [(6, 5, 5), (33, 8, 41)], ids=lambda g: "%dx%d-%d" % g)
def test_exact_stem_counts_the_set_taps(geometry):
    st = ref.states(*geometry)
    y = ref.exact_stem_of(geometry, "directed")
    assert y.dtype == np.float64 and y.shape == (len(st), 16, (st.H + 1) // 2, (st.W + 1) // 2)
    for k in range(len(st)):
        assert np.array_equal(y[k, 1], _brute_force_count(st, k).astype(np.float64)), k
    assert not y[:, 0].any() and (y[:, 2] <= -3).all() and np.array_equal(y[:, 5], np.ones_like(y[:, 5]))


@pytest.mark.parametrize("geometry", ref.GEOMETRIES, ids=lambda g: "%dx%d-%d" % g)
def test_exact_stem_agrees_with_float32_pytorch(geometry):
    import torch
    import torch.nn.functional as F
    W, H, N = geometry
    st = ref.states(W, H, N)
    w, b = ref.module_weights(N)
    with torch.no_grad():
        y32 = F.max_pool2d(F.conv2d(torch.from_numpy(st.planes()), torch.from_numpy(w.copy()), torch.from_numpy(b.copy()), padding=1), 3, 2, 1).numpy()
    assert np.abs(y32.astype(np.float64) - ref.exact_stem_of(geometry, "module")).max() <= 1e-5


def test_stem_bound_of_the_directed_channels():
    for N in (1, 32, 128):
        B, q = ref.stem_bound_of(N, "directed")
        assert B[0] == 0.0 and q[0] == 2.0 ** -40
        zero = np.zeros((1, 16, 1, 1))
        assert ref.stem_tolerance(B, q, N, zero, zero)[0, 0, 0, 0] == (N + 2) * 2.0 ** -41 + 0.5 * 2.0 ** -149
        assert B[1] == 9.0 * (N + 1) and B[2] == 9.0 * (N + 1) + 3.0 and B[5] == 1.0 and q[5] == 2.0 ** -29
        assert B[3] >= 2.0 ** 20 and B[3] == np.floor(B[3])
        assert q[4] == max(B[4] * 2.0 ** -29, 2.0 ** -40) and B[4] < 2.0 ** -8
    B, q = ref.stem_bound_of(1, "directed")
    assert B[4] < 2.0 ** -11 and q[4] == 2.0 ** -40  # the cap applies
    assert ref.ulp32(1.0) == 2.0 ** -23 and ref.ulp32(0.75) == 2.0 ** -24 and ref.ulp32(0.0) == 2.0 ** -149 and ref.ulp32(-3.0) == 2.0 ** -22
