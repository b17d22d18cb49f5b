"""Packings out of the batched engine: `pack()` plays a set of instances greedily with a network at batched speed and returns
every instance's layout as a `Packing`; the same records come out of `BatchedSelfPlay(..., record_packings=True).pop_packings()`.

The engine records a move as (action, rows): action = item * W + column (BinPackingGame.py:67) and rows = the mask of the bin rows
whose cells [x, x + w) the move filled.  `Bin.execute_move` (BinPackingLogic.py:95-109) fills the first h FREE row segments scanning
from row 0, so a move's rows may be non-contiguous, and fewer than h where the strip runs out; a single `y` would lose that.  The
views below are host NumPy over a few bytes per move.  `str(packing)` stands in for the reference's `display(board)`
(BinPackingGame.py:232), which prints an Othello board.
"""
import numpy as np

from . import _lib

_SYMBOLS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _opt(args, name, default):
    try:
        return getattr(args, name)
    except (AttributeError, KeyError):
        return default


class Packing:
    """One finished episode: which item went to which column, which bin rows it landed in, and the bin it left.

    Plain data: episode_id, W, item_wh uint8 [N, 2] (w, h), actions int32 [moves], rows uint64 [moves] (bit r = bin row r),
    board uint64 [H] (bit c of board[r] = cell (r, c)), outcome (+-1, the ranked result), score."""

    def __init__(self, episode_id, W, item_wh, actions, rows, board, outcome=0, score=0.0):
        self.episode_id = int(episode_id)
        self.W = int(W)
        self.item_wh = np.ascontiguousarray(item_wh, dtype=np.uint8).reshape(-1, 2)
        self.actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        self.board = np.ascontiguousarray(board, dtype=np.uint64).reshape(-1)
        self.outcome, self.score = int(outcome), float(score)
        if self.actions.shape != self.rows.shape:
            raise ValueError("one rows mask per action")
        if len(self.actions) and (self.actions.min() < 0 or self.actions.max() >= self.W * len(self.item_wh)):
            raise ValueError("action outside the %d x %d action space" % (len(self.item_wh), self.W))

    # ---- sizes ---------------------------------------------------------------------------------------
    @property
    def H(self):
        return len(self.board)

    @property
    def N(self):
        return len(self.item_wh)

    @property
    def moves(self):
        return len(self.actions)

    # ---- per move ------------------------------------------------------------------------------------
    @property
    def item(self):
        return self.actions // self.W

    @property
    def x(self):
        return self.actions % self.W

    def _row_bits(self):
        """bool [moves, H]: move m filled bin row r."""
        r = np.arange(self.H, dtype=np.uint64)
        return ((self.rows[:, None] >> r[None, :]) & np.uint64(1)).astype(bool)

    @property
    def n_rows(self):
        """Rows each move filled: the item's h, or fewer where the strip ran out."""
        return self._row_bits().sum(axis=1).astype(np.int32)

    @property
    def y(self):
        """Lowest bin row each move filled (-1 for a move that filled none)."""
        bits = self._row_bits()
        return np.where(bits.any(axis=1), bits.argmax(axis=1), -1).astype(np.int32)

    @property
    def contiguous(self):
        """bool [moves]: the filled rows are one run y .. y + n_rows - 1 (the item kept its shape; it may still be cut short, down
        to no row at all when every segment under it is taken: the item is discarded, BinPackingGame.py:193-195)."""
        bits = self._row_bits()
        top = np.where(bits.any(axis=1), self.H - 1 - bits[:, ::-1].argmax(axis=1), -2)
        return (top - self.y + 1) == self.n_rows

    @property
    def partial(self):
        """bool [moves]: fewer rows were filled than the item is high."""
        return self.n_rows < self.item_wh[self.item, 1].astype(np.int32)

    def _span(self, m):
        x, w = int(self.x[m]), int(self.item_wh[self.item[m], 0])
        if x + w > self.W:
            raise ValueError("move %d: item %d (width %d) at column %d leaves the %d-wide bin" % (m, self.item[m], w, x, self.W))
        return np.uint64(((1 << w) - 1) << x)

    # ---- boards --------------------------------------------------------------------------------------
    def board_after(self, m):
        """Row masks uint64 [H] of the bin after moves 0..m (m = -1: the empty bin)."""
        out = np.zeros(self.H, np.uint64)
        if m >= self.moves:
            raise IndexError("the episode has %d moves" % self.moves)
        bits = self._row_bits()
        for k in range(m + 1):
            out[bits[k]] |= self._span(k)
        return out

    @property
    def height(self):
        """get_minimal_bin_height (BinPackingGame.py:181-186) of the final bin: the highest used row + 1, 1 for an empty bin."""
        used = np.flatnonzero(self.board)
        return int(used[-1]) + 1 if len(used) else 1

    def layout(self):
        """int8 [H, W]: index of the item that occupies each cell, -1 where the bin is empty.  Raises ValueError if two moves claim
        one cell or if the cells of all moves are not exactly the final board."""
        out = np.full((self.H, self.W), -1, np.int8)
        bits = self._row_bits()
        for m in range(self.moves):
            self._span(m)
            x, w, it = int(self.x[m]), int(self.item_wh[self.item[m], 0]), int(self.item[m])
            for r in np.flatnonzero(bits[m]):
                if (out[r, x:x + w] >= 0).any():
                    raise ValueError("move %d (item %d) overlaps item %d in row %d" % (m, it, int(out[r, x:x + w].max()), r))
                out[r, x:x + w] = it
        cols = np.arange(self.W, dtype=np.uint64)
        final = ((self.board[:, None] >> cols[None, :]) & np.uint64(1)).astype(bool)
        if not np.array_equal(out >= 0, final):
            raise ValueError("the moves' cells differ from the final board in %d cells" % int(((out >= 0) != final).sum()))
        return out

    def __str__(self):
        lay = self.layout()
        sym = lambda i: "." if i < 0 else (_SYMBOLS[i] if i < len(_SYMBOLS) else "#")
        head = "episode %d: %d of %d items placed, height %d of %d, score %.4f, outcome %+d" % (
            self.episode_id, self.moves, self.N, self.height, self.H, self.score, self.outcome)
        body = ["%3d |%s|" % (r, "".join(sym(int(c)) for c in lay[r])) for r in range(self.H - 1, -1, -1)]  # row 0 at the bottom
        return "\n".join([head] + body + ["    +" + "-" * self.W + "+"])

    def __repr__(self):
        return "Packing(episode_id=%d, moves=%d, height=%d, score=%r)" % (self.episode_id, self.moves, self.height, self.score)

    def __eq__(self, other):
        return (isinstance(other, Packing) and self.episode_id == other.episode_id and self.W == other.W and self.outcome == other.outcome
                and self.score == other.score and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("item_wh", "actions", "rows", "board")))

    __hash__ = None


def greedy_rule(args):
    """The engine move rule of greedy play (greedy_a == 0, MCTS_bpp.py:43-49) under args.greedy_tie_break."""
    tie = _opt(args, "greedy_tie_break", "lowest")
    if tie not in ("lowest", "draw"):
        raise ValueError("args.greedy_tie_break must be 'lowest' or 'draw', not %r" % (tie,))
    return _lib.MOVE_ARGMAX_DRAW if tie == "draw" else _lib.MOVE_ARGMAX_FIRST


def play_packings(sp, item_wh=None, seeds=None, total_area=None, bin_h=None, bin_w=None, rewards_list=(), first_id=0):
    """Plays the instances through the driver `sp` (record_packings on) -> list[Packing] in instance order.  The driver's finished
    ring holds four records per slot, so larger pools are played in runs of two per slot."""
    if (item_wh is None) == (seeds is None):
        raise ValueError("give either item_wh or seeds")
    if not sp.record_packings:
        raise RuntimeError("the driver was built without record_packings")
    n = len(item_wh) if seeds is None else len(seeds)
    sp.pop_packings()
    out = []
    run = max(1, 2 * min(g.G for g in sp.groups) * len(sp.groups))
    for lo in range(0, n, run):
        hi = min(n, lo + run)
        if seeds is None:
            wh = np.ascontiguousarray(item_wh, dtype=np.uint8)[lo:hi]
            if total_area is None:
                area = (wh[:, :, 0].astype(np.int32) * wh[:, :, 1]).sum(axis=1).astype(np.int32)
            else:
                area = np.asarray(total_area, np.int32).reshape(-1)[lo:hi]
            sp.run(wh, area, rewards_list, first_id=first_id + lo)
        else:
            sp.run_from_seeds(np.asarray(seeds, dtype=np.uint32)[lo:hi], rewards_list, first_id=first_id + lo, bin_h=bin_h, bin_w=bin_w)
        got = sp.pop_packings()
        if [p.episode_id for p in got] != list(range(first_id + lo, first_id + hi)):
            raise RuntimeError("instances %d..%d: %d packings came back" % (lo, hi - 1, len(got)))
        out += got
    return out


def pack(game, nnet, args, item_wh=None, seeds=None, bin_h=None, move_rule=None, rewards_list=(), total_area=None, bin_w=None, games=None,
         driver=None, seed=0, **driver_kw):
    """Packs every instance with `nnet` guiding args.numMCTSSims simulations per move -> list[Packing] in instance order
    (episode_id = the instance's index).

    item_wh: uint8 [n, N, 2] item sizes (w, h), total area = the items' own unless total_area [n] is given; or seeds [n]: instance i =
    ItemsGenerator.items_generator(seeds[i]) of the bin_w x bin_h rectangle (default: the board) cut on the device, total area
    bin_w * bin_h (CoachBPP.py:119).  move_rule: default greedy per args.greedy_tie_break, as the reference's arena plays
    (greedy_a=0, CoachBPP.py:259); rewards_list: the R2 buffer the outcomes are ranked against.  A packing's score is not a function of
    it, but the search is: a terminal's value is its outcome against the buffer (and, on a tie, driver_kw's tie_salt), so another
    buffer can choose other moves.
    games: concurrent slots (default min(n, 4096)); more instances than slots go through the engine's auto-restart.
    driver: a BatchedSelfPlay with record_packings=True to reuse (its move rule is set; it is left open); otherwise one is built
    with **driver_kw, records no training examples (max_examples=0) and is closed afterwards.
    Network-free: pack(game, None, args, evaluator="rollout", playouts=K, rewards_list=...) searches with uniform priors and the mean
    outcome of K random playouts per leaf (BatchedSelfPlay's evaluator="rollout").  The playouts are ranked against rewards_list too: with
    an empty list every outcome is +1 and the search is blind, so a network-free solve wants a buffer -- random_scores() gives one."""
    from .selfplay import BatchedSelfPlay
    n = len(item_wh) if seeds is None else len(seeds)
    rule = greedy_rule(args) if move_rule is None else int(move_rule)
    sp = driver
    if sp is None:
        games = int(games or min(max(n, 1), 4096))
        driver_kw.setdefault("groups", max(1, min(2, games)))
        sp = BatchedSelfPlay(game, nnet, args, games=games, move_rule=rule, seed=seed, max_examples=0, record_packings=True, **driver_kw)
    elif sp.move_rule != rule:
        sp.set_move_rule(rule)
    try:
        return play_packings(sp, item_wh=item_wh, seeds=seeds, total_area=total_area, bin_h=bin_h, bin_w=bin_w, rewards_list=rewards_list)
    finally:
        if driver is None:
            sp.close()


def random_scores(game, item_wh=None, seeds=None, playouts=16, seed=0, bin_h=None, bin_w=None):
    """Scores of uniform random packings -> float64 [n, playouts]: `playouts` random playouts of every instance from the empty bin
    (rp_rollout_states; instance i plays as episode i, playout j draws from (seed, i, j)).  The random baseline a search or a trained
    network is compared with, and -- flattened -- a first R2 buffer for pack(..., evaluator="rollout", rewards_list=...).
    item_wh / seeds / bin_h / bin_w: the instances, as pack() takes them."""
    if (item_wh is None) == (seeds is None):
        raise ValueError("give either item_wh or seeds")
    W, H, N = game.bin_width, game.bin_height, game.num_items
    eng = _lib.Engine(W, H, N, 1, 1, seed=int(seed) & 0x7FFFFFFFFFFFFFFF)
    try:
        if seeds is not None:
            item_wh = eng.generate_items(seeds, bin_w=bin_w, bin_h=bin_h)
            area = np.full(len(item_wh), int(bin_w or W) * int(bin_h or H), np.int32)
        else:
            item_wh = np.ascontiguousarray(item_wh, dtype=np.uint8).reshape(-1, N, 2)
            area = (item_wh[:, :, 0].astype(np.int32) * item_wh[:, :, 1]).sum(axis=1).astype(np.int32)
        n = len(item_wh)
        if n == 0:
            return np.zeros((0, int(playouts)), np.float64)
        max_h = item_wh[:, :, 1].max(axis=1).astype(np.int32)
        _, score, _, _ = eng.rollout_states(np.zeros((n, H), np.uint64), np.ones((n, N), np.uint8), item_wh, area, max_h, (), 0.75, playouts,
                                            episode_id=np.arange(n, dtype=np.uint64), boards=False)
        return score
    finally:
        eng.close()
