"""Chosen states, stem weights and float64 references for the three leaf-input kernels: k_leaf_stem (with k_stem_tables),
k_leaf_planes and k_examples.  Host code only: test_leaf_inputs_cpu.py checks what is built here, test_gpu_leaf_inputs.py drives
the kernels with it.

The states need not be reachable by play (rp_set_roots and rp_expand_examples take any state), but every one of them has a legal
move by construction: item 0 is 1x1 and unplaced and column 0 has a free cell.  Column 0 always counts as adjacent
(oracle/rp_oracle.c, adjacency) and a w x h item is legal there when the occupied cells of columns 0..w-1 number at most w (H - h)
(moves_for_item), so a 1x1 item at column 0 is legal whenever column 0 has a free cell.  The full board is terminal: every window
holds H w occupied cells, more than w (H - h).

Everything is drawn from SEED and cached: callers share one copy (read-only arrays) and must not change it."""
import functools

import numpy as np

import evaluators as ev
from engine_util import planes_from_state

SEED = 20261020
# (W, H, N), each for a boundary of k_leaf_stem: the degenerate ends, Wp < 4 (corner columns CC = 2 Wp), the production board, the
# item table's last size in LDS (N = 40) and first in L2 (N = 41, with the first 64-bit row, W = 33), Wp = 32 at H = 1, the second
# item word (N = 65) with a row in every lane (H = 64), and the ABI's limits
GEOMETRIES = [(1, 1, 1), (2, 3, 4), (6, 5, 5), (20, 20, 32), (32, 9, 40), (33, 8, 41), (64, 1, 3), (12, 64, 65), (63, 64, 64), (64, 64, 128)]
STATES_PER_GEOMETRY = 16
TILE_GEOMETRY = (64, 64, 128)  # carries two more states whose boards hold every 3x3 pattern as a tile
INTEGER_CHANNELS = (0, 1, 2, 3, 5)  # of the directed weight set: their sums are small integers times a power of two
CORNER_MIN_ITEMS = 4  # k_leaf_stem takes the corner phase with this many small unplaced items or more


class States:
    """S states of one geometry: rows uint64 [S, H], rem uint8 [S, N], wh uint8 [S, N, 2] (w, h)."""

    def __init__(self, W, H, N, rows, rem, wh):
        self.W, self.H, self.N = W, H, N
        self.rows, self.rem, self.wh = rows, rem, wh
        for a in (rows, rem, wh):
            a.setflags(write=False)

    def __len__(self):
        return len(self.rows)

    def board(self, k):
        return ev.unpack_board(self.rows[k], self.W)

    def planes(self, idx=None):
        idx = range(len(self)) if idx is None else idx
        return np.stack([planes_from_state(self.rows[k], self.rem[k], self.wh[k], self.W, self.H) for k in idx])


# ---- the launcher's and the kernel's own arithmetic (rp_leaf_stem, k_leaf_stem) ----------------------------------------------
def corner_dims(W):
    """(CR, CC) of the corner phase: nprf = min(4, 60 / Wp + 1), CR = min(8, 2 nprf), CC = 2 min(4, Wp)."""
    Wp = (W + 1) // 2
    nprf = min(4, 60 // Wp + 1)
    return min(8, 2 * nprf), min(8, 2 * min(4, Wp))


def small_items(rem, wh, W):
    """Number of items the kernel counts for the corner phase: unplaced, h < CR, w < CC."""
    CR, CC = corner_dims(W)
    return int(((np.asarray(rem) != 0) & (wh[:, 1] < CR) & (wh[:, 0] < CC)).sum())


def table_in_lds(N):
    """rp_leaf_stem keeps the item table ((25 N + 1) rows of 16 ints) in LDS while it fits 64 KB."""
    return (N * 25 + 1) * 16 * 4 <= 64 * 1024


def stem_passes(W, H):
    """Number of 64-lane passes of one leaf: the first stores 64 pooled pixels, every other one 63 - Wp."""
    Wp, P = (W + 1) // 2, ((W + 1) // 2) * ((H + 1) // 2)
    base = passes = 0
    while base + (Wp + 1 if passes else 0) < P:
        base += 63 - Wp
        passes += 1
    return passes


# ---- states ------------------------------------------------------------------------------------------------------------------
def _boards(W, H, rng):
    """The seven board kinds, each with a free cell in column 0."""
    r, c = np.indices((H, W))
    out = [np.zeros((H, W), np.uint8)]
    out += [(rng.random((H, W)) < dens).astype(np.uint8) for dens in (0.15, 0.5, 0.9)]
    out.append(((r + c) & 1).astype(np.uint8))  # checkerboard, cell (0, 0) free
    full = np.ones((H, W), np.uint8)
    full[:, 0] = 0
    out.append(full)
    edge = np.zeros((H, W), np.uint8)
    edge[:, W - 1] = 1
    edge[H - 1, :] = 1
    out.append(edge)
    for b in out:
        if b[:, 0].all():
            b[0, 0] = 0
    return out


def _special_sizes(W, H):
    out = [(W, H), (W, 1), (1, H), (1, 1)]
    out += [(a, b) for a in (7, 8, 9) for b in (7, 8, 9) if a <= W and b <= H]
    out += [(a, min(H, 2)) for a in (7, 8, 9) if a <= W] + [(min(W, 2), b) for b in (7, 8, 9) if b <= H]
    return out


def _items(W, H, N, s, rng):
    """Item sizes of state s: item 0 is 1x1, the next ones walk through the special sizes (rotated with s, so that small N see
    them all over the 16 states), the rest are random, half of them at most 9 wide and high."""
    wh = np.empty((N, 2), np.int64)
    wh[:, 0] = rng.integers(1, W + 1, N)
    wh[:, 1] = rng.integers(1, H + 1, N)
    low = rng.random(N) < 0.5
    wh[low, 0] = rng.integers(1, min(W, 9) + 1, int(low.sum()))
    wh[low, 1] = rng.integers(1, min(H, 9) + 1, int(low.sum()))
    special = _special_sizes(W, H)
    for i in range(1, min(N, len(special) + 1)):
        wh[i] = special[(s * (N - 1) + i - 1) % len(special)]
    wh[0] = (1, 1)
    return wh


def _remaining(W, H, N, kind, wh, rng):
    """kind 0 all items, 1 item 0 alone, 2 a random half, 3 at least four small items (sizes of items 1..5 redrawn below the
    corner), 4 at most three small items.  Item 0 always takes part.  May change wh (kind 3)."""
    CR, CC = corner_dims(W)
    rem = np.ones(N, np.uint8)
    if kind == 1:
        rem[1:] = 0
    elif kind == 2:
        rem = (rng.random(N) < 0.5).astype(np.uint8)
    elif kind == 3:
        for i in range(1, min(N, 6)):
            wh[i] = (rng.integers(1, min(CC - 1, W) + 1), rng.integers(1, min(CR - 1, H) + 1))
        rem = (rng.random(N) < 0.7).astype(np.uint8)
        rem[:6] = 1
    elif kind == 4:
        rem = (rng.random(N) < 0.6).astype(np.uint8)
        small = np.nonzero((wh[:, 1] < CR) & (wh[:, 0] < CC))[0]
        rem[small[3:]] = 0  # item 0 is small and comes first: it stays
    rem[0] = 1
    return rem


def _tile_boards():
    """Two 64x64 boards: tile k of 256 occupies rows 4i..4i+2 and columns 4j..4j+2 (k = 16 i + j) and shows pattern k (board 0)
    or 256 + k (board 1), bit 3 dr + dx = cell (4i + dr, 4j + dx) -- the pattern the convolution output at the tile's centre
    sees.  Row 4i+3 and column 4j+3 stay empty."""
    out = []
    for half in range(2):
        b = np.zeros((64, 64), np.uint8)
        for k in range(256):
            i, j, pat = k // 16, k % 16, 256 * half + k
            for bit in range(9):
                b[4 * i + bit // 3, 4 * j + bit % 3] = (pat >> bit) & 1
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def states(W, H, N, count=STATES_PER_GEOMETRY):
    """The geometry's states: board kind s % 7 with remaining-set kind s % 5 for state s (all pairs differ below 35 states)."""
    rng = np.random.default_rng([SEED, W, H, N, count])
    rows, rem, whs = [], [], []
    boards = []
    for s in range(count):
        boards.append((_boards(W, H, rng)[s % 7], s % 5))
    if (W, H, N) == TILE_GEOMETRY:
        boards += [(b, k) for b, k in zip(_tile_boards(), (0, 2))]
    for s, (board, rem_kind) in enumerate(boards):
        wh = _items(W, H, N, s, rng)
        rem.append(_remaining(W, H, N, rem_kind, wh, rng))
        whs.append(wh.astype(np.uint8))
        rows.append(ev.pack_board(board))
    return States(W, H, N, np.stack(rows).astype(np.uint64), np.stack(rem).astype(np.uint8), np.stack(whs))


def terminal_rows(W, H):
    """The full board: no item has a legal move on it."""
    return np.full(H, (1 << W) - 1, np.uint64)


PIPELINE_GEOMETRY = (10, 10, 8)  # the look-ahead test: many slots filled from PIPELINE_STATES distinct states
PIPELINE_STATES = 64


def pipeline_slots(games):
    """-> (state of every slot: the distinct states repeated in a shuffled order, mask of the slots that hold the terminal full
    board instead: every seventh)."""
    rng = np.random.default_rng([SEED, games, 3])
    order = rng.permutation(np.arange(games) % PIPELINE_STATES)
    return order, np.arange(games) % 7 == 6


def persistent_trips(games, n_cu, stem_waves=3, waves_per_block=4):
    """Largest number of leaves one wave of the LDS form of k_leaf_stem loops over: rp_leaf_stem launches at most n_cu x STEM_WAVES
    workgroups of WAVES_PER_BLOCK waves, a wave per leaf, stride = the grid's waves."""
    grid = min(-(-games // waves_per_block), n_cu * stem_waves)
    return -(-games // (grid * waves_per_block))


def grid_patterns(board):
    """[H, W] of the 3x3 bit pattern around every cell, bit 3 dr + dx = cell (r + dr - 1, x + dx - 1), zero outside the grid --
    the index of the stem's grid table TB at that convolution output."""
    H, W = board.shape
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = board
    pat = np.zeros((H, W), np.int64)
    for dr in range(3):
        for dx in range(3):
            pat |= pad[dr:dr + H, dx:dx + W] << (3 * dr + dx)
    return pat


# ---- weight sets [16][N+1][3][3], bias [16] ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directed_weights(N):
    rng = np.random.default_rng([SEED, N, 1])
    w = rng.standard_normal((16, N + 1, 3, 3))  # channels 6 to 15: normal(0, 1)
    b = rng.standard_normal(16)
    w[0], b[0] = 0.0, 0.0                         # zero bound: the unit is the cap, 2^-40
    w[1], b[1] = 1.0, 0.0                         # counts the set taps
    w[2], b[2] = -1.0, -3.0                       # negative everywhere: outputs outside an odd image must lose every maximum
    w[3], b[3] = rng.integers(-3, 4, (N + 1, 3, 3)) * 2.0 ** 20, rng.integers(-3, 4) * 2.0 ** 20  # a large bound
    w[4], b[4] = rng.standard_normal((N + 1, 3, 3)) * 2.0 ** -20, rng.standard_normal() * 2.0 ** -20  # a small one (cap for bounds < 2^-11)
    w[5], b[5] = 0.0, 1.0                         # bound exactly a power of two
    w, b = w.astype(np.float32), b.astype(np.float32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


@functools.lru_cache(maxsize=None)
def module_weights(N):
    """torch.nn.Conv2d(N + 1, 16, 3, padding=1) as it initialises itself, from a fixed seed (the global generator is left alone)."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(SEED + N)
        conv = torch.nn.Conv2d(N + 1, 16, 3, padding=1)
    w, b = conv.weight.detach().numpy().copy(), conv.bias.detach().numpy().copy()
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


WEIGHT_SETS = {"directed": directed_weights, "module": module_weights}


# ---- references ----------------------------------------------------------------------------------------------------------------
def exact_stem(st, w, b):
    """max_pool2d(conv2d(planes, w, b, padding=1), 3, 2, 1) in float64 on the CPU, planes from planes_from_state; not rounded."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(st.planes()).double()
    with torch.no_grad():
        y = F.conv2d(x, torch.from_numpy(np.array(w, np.float64)), torch.from_numpy(np.array(b, np.float64)), padding=1)
        return F.max_pool2d(y, kernel_size=3, stride=2, padding=1).numpy()


@functools.lru_cache(maxsize=None)
def exact_stem_of(geometry, weight_set):
    """exact_stem of the geometry's states under one of WEIGHT_SETS, computed once."""
    W, H, N = geometry
    y = exact_stem(states(W, H, N), *WEIGHT_SETS[weight_set](N))
    y.setflags(write=False)
    return y


_INTERVALS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)]  # taps [lb, ub] of one axis that a run of ones anchored at the origin can cover


def stem_bound(w, b, N):
    """include/rp_engine.h's accuracy contract of rp_leaf_stem on the host, float64, per output channel o -> (B [16], q [16]).

    B_o = max(P, M): P (M) is the positive (negative) part of the bias + the largest (smallest) of the 512 grid-pattern sums + for
    each item the largest (smallest) of its 25 class sums -- no reachable sum of table entries exceeds it.  The classes are the
    sub-rectangles of the 3x3 taps that a rectangle anchored at the origin can cover: 5 tap intervals per axis.  k_stem_tables
    takes the unit 2^-k with k = 30 - ex, bound < 2^ex, capped at 40: as B_o >= 2^(ex-1), the unit q_o <= max(B_o 2^-29, 2^-40)."""
    w = np.asarray(w, np.float64)
    b = np.asarray(b, np.float64)
    B, q = np.zeros(16), np.zeros(16)
    for o in range(16):
        hi = lo = 0.0
        for pat in range(512):
            v = 0.0
            for tap in range(9):
                if (pat >> tap) & 1:
                    v += w[o, 0, tap // 3, tap % 3]
            hi, lo = max(hi, v), max(lo, -v)
        P, M = max(b[o], 0.0) + hi, max(-b[o], 0.0) + lo
        for i in range(N):
            hi = lo = 0.0
            for rlb, rub in _INTERVALS:
                for clb, cub in _INTERVALS:
                    v = 0.0
                    for dr in range(rlb, rub + 1):
                        for dx in range(clb, cub + 1):
                            v += w[o, i + 1, dr, dx]
                    hi, lo = max(hi, v), max(lo, -v)
            P += hi
            M += lo
        B[o] = max(P, M)
        q[o] = max(B[o] * 2.0 ** -29, 2.0 ** -40)
    return B, q


@functools.lru_cache(maxsize=None)
def stem_bound_of(N, weight_set):
    return stem_bound(*WEIGHT_SETS[weight_set](N), N)


def ulp32(x):
    """Spacing of float32 at |x| (float64 in, float64 out; the smallest subnormal at zero)."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)  # |x| = m 2^e, 0.5 <= m < 1 (e = 0 at zero)
    return np.ldexp(1.0, np.where(x == 0.0, -149, np.maximum(e - 24, -149)))


def stem_tolerance(B, q, N, y, g):
    """Absolute bound on |g - y| for exact results y [S, 16, Hp, Wp] (float64) and kernel results g: (N + 2) q_o / 2 for the
    quantised table entries (bias, grid pattern, N items), half an ulp32 of max(|y|, |g|) for the one int-to-float conversion and
    9 (N + 1) 2^-53 B_o for the float64 reference's own rounding."""
    B, q = B.reshape(1, 16, 1, 1), q.reshape(1, 16, 1, 1)
    big = np.maximum(np.abs(np.asarray(y, np.float64)), np.abs(np.asarray(g, np.float64)))
    return (N + 2) * q / 2 + 0.5 * ulp32(big) + 9 * (N + 1) * 2.0 ** -53 * B


# ---- packed replay sets (include/rp_engine.h, rp_examples_packed) --------------------------------------------------------------
def key_words(W, H, N):
    KW = H * (2 if W > 32 else 1) + (N + 31) // 32
    return KW + 1 if W > 32 and KW % 2 else KW


def pack_keys(st):
    """uint32 [S, KW]: H row masks (u32 for W <= 32, else u64, little endian) then ceil(N / 32) words of remaining-item bits."""
    W, H, N, S = st.W, st.H, st.N, len(st)
    RW = 2 if W > 32 else 1
    key = np.zeros((S, key_words(W, H, N)), np.uint32)
    if RW == 2:
        key[:, :2 * H] = np.ascontiguousarray(st.rows.astype("<u8")).view("<u4").reshape(S, 2 * H)
    else:
        key[:, :H] = st.rows.astype(np.uint32)
    for i in range(N):
        key[:, H * RW + i // 32] |= (st.rem[:, i] != 0).astype(np.uint32) << np.uint32(i % 32)
    return key


@functools.lru_cache(maxsize=None)
def packed_set(W, H, N):
    """A packed replay set of the geometry's states, one example per state -> dict of arrays in the header's layout (sp_off 64-bit,
    as rp_expand_examples takes it).  Example 1 has no visit counts (sp_n = 0); the counts reach 2^32 - 1; an example has up to 70
    pairs where the action space allows, more than one 64-lane trip."""
    st = states(W, H, N)
    rng = np.random.default_rng([SEED, W, H, N, 2])
    E, A = len(st), W * N
    sp_n = rng.integers(1, min(A, 70) + 1, E).astype(np.int32)
    sp_n[0] = min(A, 70)
    sp_n[1] = 0
    sp_off = np.concatenate([[0], np.cumsum(sp_n)[:-1]]).astype(np.int64)
    acts, cnts = [], []
    for e in range(E):
        acts.append(np.sort(rng.choice(A, size=int(sp_n[e]), replace=False)))
        c = rng.integers(1, 50, int(sp_n[e]))
        big = rng.random(int(sp_n[e])) < 0.3
        c[big] = rng.integers(1, 1 << 32, int(big.sum()))
        cnts.append(c)
    cnts[0][0] = (1 << 32) - 1
    d = dict(key=pack_keys(st), wh=st.wh.copy(), value=rng.integers(-1, 2, E).astype(np.int32), sp_off=sp_off, sp_n=sp_n,
             sp_act=np.concatenate(acts).astype(np.uint16), sp_cnt=np.concatenate(cnts).astype(np.uint32))
    for a in d.values():
        a.setflags(write=False)
    return d


def expected_pi(d, A, e):
    """float32 [A]: float32(float64(count) / float64(sum of the example's counts)), zero elsewhere (MCTS_bpp.py:51-54)."""
    off, n = int(d["sp_off"][e]), int(d["sp_n"][e])
    pi = np.zeros(A, np.float32)
    if n:
        c = d["sp_cnt"][off:off + n].astype(np.float64)
        pi[d["sp_act"][off:off + n]] = (c / float(c.sum())).astype(np.float32)
    return pi
