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
    board uint64 [H] (bit c of board[r] = cell (r, c)), outcome (+-1, the ranked result), score; and where the episode started
    (rp_set_instance_initial): initial_board uint64 [H], the cells set before the first move (default: none), and present bool [N],
    the items that took part (default: all).

    An incumbent (pack(..., best=True), BatchedSelfPlay.pop_best_packings) is a Packing too: the best complete packing the episode's search
    tree saw.  It also carries prefix (how many of its moves had been played when the search found it), updates (how often the episode's
    incumbent was replaced, the first entry included) and played (the Packing the move rule played, where it was recorded); all three
    are None on a played Packing.  Under playout incumbents (pack(..., playout_incumbents=True)) it also says where it came from:
    tree_moves (the number of actions after which the search tree was left) and playout (the index of the random playout that made the
    remaining moves, -1 for a terminal of the tree, whose tree_moves == moves); None otherwise."""
    prefix = updates = played = tree_moves = playout = None

    def __init__(self, episode_id, W, item_wh, actions, rows, board, outcome=0, score=0.0, initial_board=None, present=None):
        self.episode_id = int(episode_id)
        self.W = int(W)
        self.item_wh = np.ascontiguousarray(item_wh, dtype=np.uint8).reshape(-1, 2)
        self.actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1)
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        self.board = np.ascontiguousarray(board, dtype=np.uint64).reshape(-1)
        self.outcome, self.score = int(outcome), float(score)
        self.initial_board = (np.zeros(len(self.board), np.uint64) if initial_board is None
                              else np.ascontiguousarray(initial_board, dtype=np.uint64).reshape(-1))
        self.present = (np.ones(len(self.item_wh), bool) if present is None else np.asarray(present).reshape(-1) != 0)
        if self.initial_board.shape != self.board.shape or self.present.shape != (len(self.item_wh),):
            raise ValueError("initial_board must have one row mask per bin row and present one flag per item")
        if self.actions.shape != self.rows.shape:
            raise ValueError("one rows mask per action")
        if len(self.actions) and (self.actions.min() < 0 or self.actions.max() >= self.W * len(self.item_wh)):
            raise ValueError("action outside the %d x %d action space" % (len(self.item_wh), self.W))
        if len(self.actions) and not self.present[self.actions // self.W].all():
            raise ValueError("a move places an item that does not take part")

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
        """Row masks uint64 [H] of the bin after moves 0..m (m = -1: the initial board, the empty bin by default)."""
        out = self.initial_board.copy()
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
        """int8 [H, W]: index of the item that occupies each cell, -1 where the bin is empty, -2 where the initial board had the cell
        set.  Raises ValueError if two moves claim one cell, if a move claims an initially set cell, or if the cells of all moves and
        the initial board are not exactly the final board."""
        out = np.full((self.H, self.W), -1, np.int8)
        cols = np.arange(self.W, dtype=np.uint64)
        out[((self.initial_board[:, None] >> cols[None, :]) & np.uint64(1)).astype(bool)] = -2
        bits = self._row_bits()
        for m in range(self.moves):
            self._span(m)
            x, w, it = int(self.x[m]), int(self.item_wh[self.item[m], 0]), int(self.item[m])
            for r in np.flatnonzero(bits[m]):
                if (out[r, x:x + w] >= 0).any():
                    raise ValueError("move %d (item %d) overlaps item %d in row %d" % (m, it, int(out[r, x:x + w].max()), r))
                if (out[r, x:x + w] == -2).any():
                    raise ValueError("move %d (item %d) claims an initially set cell in row %d" % (m, it, r))
                out[r, x:x + w] = it
        final = ((self.board[:, None] >> cols[None, :]) & np.uint64(1)).astype(bool)
        if not np.array_equal(out != -1, final):
            raise ValueError("the moves' and the initial board's cells differ from the final board in %d cells" % int(((out != -1) != final).sum()))
        return out

    def __str__(self):
        lay = self.layout()
        sym = lambda i: "." if i == -1 else (_SYMBOLS[i] if 0 <= i < len(_SYMBOLS) else "#")  # '#': an initially set cell (or item 62+)
        head = "episode %d: %d of %d items placed, height %d of %d, score %.4f, outcome %+d" % (
            self.episode_id, self.moves, int(self.present.sum()), self.height, self.H, self.score, self.outcome)
        body = ["%3d |%s|" % (r, "".join(sym(int(c)) for c in lay[r])) for r in range(self.H - 1, -1, -1)]  # row 0 at the bottom
        return "\n".join([head] + body + ["    +" + "-" * self.W + "+"])

    def __repr__(self):
        return "Packing(episode_id=%d, moves=%d, height=%d, score=%r)" % (self.episode_id, self.moves, self.height, self.score)

    def __eq__(self, other):
        return (isinstance(other, Packing) and self.episode_id == other.episode_id and self.W == other.W and self.outcome == other.outcome
                and self.score == other.score and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("item_wh", "actions", "rows", "board", "initial_board", "present")))

    __hash__ = None


def replay_rows(W, H, item_wh, actions, initial_board=None):
    """Bin.execute_move (BinPackingLogic.py:95-109) over a sequence of actions, on the host -> (rows uint64 [moves], board uint64 [H]):
    rows[m] = mask of the bin rows move m filled, board = the bin after the last move.  action = item * W + column; the item's cells
    [column, column + w) -- clipped at W like the NumPy slice -- go to the first h rows, scanning from row 0, in which they are all
    free; fewer than h where the bin runs out.  The engine stores an incumbent as its actions and final bin only; this gives the
    per-move rows back.  initial_board: uint64 [H] row masks (default: the empty bin)."""
    W, H = int(W), int(H)
    item_wh = np.asarray(item_wh).reshape(-1, 2)
    board = [0] * H if initial_board is None else [int(x) for x in np.asarray(initial_board, dtype=np.uint64).reshape(-1)]
    if len(board) != H:
        raise ValueError("initial_board must have one row mask per bin row")
    full = (1 << W) - 1
    rows = []
    for a in np.asarray(actions, dtype=np.int64).reshape(-1):
        i, j = divmod(int(a), W)
        if not 0 <= i < len(item_wh):
            raise ValueError("action %d outside the %d x %d action space" % (a, len(item_wh), W))
        w, h = int(item_wh[i, 0]), int(item_wh[i, 1])
        span = (((1 << w) - 1) << j) & full
        filled = 0
        for r in range(H):
            if h == 0:
                break
            if board[r] & span == 0:
                board[r] |= span
                filled |= 1 << r
                h -= 1
        rows.append(filled)
    return np.array(rows, dtype=np.uint64), np.array(board, dtype=np.uint64)


def greedy_rule(args):
    """The engine move rule of greedy play (greedy_a == 0, MCTS_bpp.py:43-49) under args.greedy_tie_break."""
    tie = _opt(args, "greedy_tie_break", "lowest")
    if tie not in ("lowest", "draw"):
        raise ValueError("args.greedy_tie_break must be 'lowest' or 'draw', not %r" % (tie,))
    return _lib.MOVE_ARGMAX_DRAW if tie == "draw" else _lib.MOVE_ARGMAX_FIRST


def initial_state(W, H, N, item_wh, initial_board=None, remaining=None):
    """The instances of pack() / random_scores() in the engine's form -> (item_wh uint8 [n, N, 2], rows uint64 [n, H] or None,
    remaining uint8 [n, N] or None, total area int32 [n]).  item_wh: [n, N, 2], or ragged -- a list of [k_i, 2] arrays with k_i <= N,
    padded with 1x1 items that do not take part.  initial_board: bool / uint8 [n, H, W] cells or uint64 [n, H] row masks; remaining:
    uint8 [n, N].  rows and remaining are None when the instances start as always: the empty bin, all items.  The area is the set
    cells of the initial board plus the area of the items that take part."""
    n = len(item_wh)
    wh = np.ones((n, N, 2), np.uint8)
    rem = np.ones((n, N), np.uint8)
    ragged = False
    if isinstance(item_wh, np.ndarray) and item_wh.shape == (n, N, 2):  # the rectangular case in one copy
        wh[:] = item_wh
        item_wh = ()
    for i, it in enumerate(item_wh):
        it = np.asarray(it, dtype=np.uint8).reshape(-1, 2)
        if len(it) > N:
            raise ValueError("instance %d has %d items, the engine is built for %d" % (i, len(it), N))
        wh[i, :len(it)] = it
        rem[i, len(it):] = 0
        ragged |= len(it) < N
    if remaining is not None:
        remaining = np.asarray(remaining)
        if remaining.shape != (n, N):
            raise ValueError("remaining must be [n, N]")
        rem &= (remaining != 0).astype(np.uint8)
    rows = None
    if initial_board is not None:
        b = np.asarray(initial_board)
        if b.ndim == 3:  # cells
            if b.shape != (n, H, W):
                raise ValueError("initial_board cells must be [n, H, W]")
            rows = ((b != 0).astype(np.uint64) << np.arange(W, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)
        else:
            rows = np.ascontiguousarray(b, dtype=np.uint64)
            if rows.shape != (n, H):
                raise ValueError("initial_board row masks must be [n, H]")
    area = (wh[:, :, 0].astype(np.int32) * wh[:, :, 1] * rem).sum(axis=1).astype(np.int32)
    if rows is not None:
        cols = np.arange(W, dtype=np.uint64)
        area = area + ((rows[:, :, None] >> cols[None, None, :]) & np.uint64(1)).sum(axis=(1, 2)).astype(np.int32)
    if rows is None and remaining is None and not ragged:
        return wh, None, None, area
    return wh, (np.zeros((n, H), np.uint64) if rows is None else rows), rem, area


def _check_instances(item_wh, seeds, initial_board, remaining):
    if (item_wh is None) == (seeds is None):
        raise ValueError("give either item_wh or seeds")
    if seeds is not None and (initial_board is not None or remaining is not None):
        raise ValueError("instances from seeds tile the bin and start empty: an initial state needs item_wh")


def play_packings(sp, item_wh=None, seeds=None, total_area=None, bin_h=None, bin_w=None, rewards_list=(), first_id=0, initial_board=None,
                  remaining=None, best=False):
    """Plays the instances through the driver `sp` (record_packings on) -> list[Packing] in instance order.  The driver's finished
    ring holds four records per slot, so larger pools are played in runs of two per slot.  initial_board / remaining / ragged item_wh:
    see pack().  best: return every instance's incumbent instead (the driver needs record_best too), its `played` the played Packing."""
    _check_instances(item_wh, seeds, initial_board, remaining)
    if not sp.record_packings:
        raise RuntimeError("the driver was built without record_packings")
    if best and not sp.record_best:
        raise RuntimeError("the driver was built without record_best")
    n = len(item_wh) if seeds is None else len(seeds)
    rows0 = rem0 = None
    if seeds is None:
        item_wh, rows0, rem0, own_area = initial_state(sp.W, sp.H, sp.N, item_wh, initial_board, remaining)
    sp.pop_packings()
    if best:
        sp.pop_best_packings()
    out = []
    run = max(1, 2 * min(g.G for g in sp.groups) * len(sp.groups))
    for lo in range(0, n, run):
        hi = min(n, lo + run)
        if seeds is None:
            wh = item_wh[lo:hi]
            area = own_area[lo:hi] if total_area is None else np.asarray(total_area, np.int32).reshape(-1)[lo:hi]
            sp.run(wh, area, rewards_list, first_id=first_id + lo, initial_rows=None if rows0 is None else rows0[lo:hi],
                   initial_remaining=None if rem0 is None else rem0[lo:hi])
        else:
            sp.run_from_seeds(np.asarray(seeds, dtype=np.uint32)[lo:hi], rewards_list, first_id=first_id + lo, bin_h=bin_h, bin_w=bin_w)
        got = sp.pop_packings()
        if [p.episode_id for p in got] != list(range(first_id + lo, first_id + hi)):
            raise RuntimeError("instances %d..%d: %d packings came back" % (lo, hi - 1, len(got)))
        if best:
            inc = sp.pop_best_packings()
            if [p.episode_id for p in inc] != [p.episode_id for p in got]:
                raise RuntimeError("instances %d..%d: %d incumbents came back" % (lo, hi - 1, len(inc)))
            for p, played in zip(inc, got):
                p.played = played
            got = inc
        out += got
    return out


def _evaluator_of(driver, driver_kw):
    """The evaluator pack() will search with: the driver's, or the one its driver will be built with."""
    return driver.evaluator if driver is not None else driver_kw.get("evaluator", "cnn")


def pack(game, nnet, args, item_wh=None, seeds=None, bin_h=None, move_rule=None, rewards_list=(), total_area=None, bin_w=None, games=None,
         driver=None, seed=0, initial_board=None, remaining=None, best=False, playout_incumbents=False, playout_policy="uniform", rollout_prior="uniform",
         playout_landing=0, **driver_kw):
    """Packs every instance with `nnet` guiding args.numMCTSSims simulations per move -> list[Packing] in instance order
    (episode_id = the instance's index).

    item_wh: uint8 [n, N, 2] item sizes (w, h), total area = the items' own unless total_area [n] is given; or seeds [n]: instance i =
    ItemsGenerator.items_generator(seeds[i]) of the bin_w x bin_h rectangle (default: the board) cut on the device, total area
    bin_w * bin_h (CoachBPP.py:119).
    Any start (item_wh only): item_wh may be ragged -- a list of [k_i, 2] arrays with k_i <= N; initial_board -- bool / uint8
    [n, H, W] cells or uint64 [n, H] row masks -- are cells taken before the first move; remaining uint8 [n, N] marks the items that
    take part.  The default total area is then the set cells plus the area of the items that take part.  An instance that has no
    legal move from its start comes back as a Packing of 0 moves.  move_rule: default greedy per args.greedy_tie_break, as the reference's arena plays
    (greedy_a=0, CoachBPP.py:259); rewards_list: the R2 buffer the outcomes are ranked against.  A packing's score is not a function of
    it, but the search is: a terminal's value is its outcome against the buffer (and, on a tie, driver_kw's tie_salt), so another
    buffer can choose other moves.
    games: concurrent slots (default min(n, 4096)); more instances than slots go through the engine's auto-restart.
    driver: a BatchedSelfPlay with record_packings=True to reuse (its move rule is set; it is left open); otherwise one is built
    with **driver_kw, records no training examples (max_examples=0) and is closed afterwards.
    Network-free: pack(game, None, args, evaluator="rollout", playouts=K, rewards_list=...) searches with uniform priors and the mean
    outcome of K random playouts per leaf (BatchedSelfPlay's evaluator="rollout").  The playouts are ranked against rewards_list too: with
    an empty list every outcome is +1 and the search is blind, so a network-free solve wants a buffer -- random_scores() gives one.
    best: return every instance's incumbent instead of the packing that was played: the best complete packing the episode's search tree
    saw (rp_set_incumbent; the first found among equals), with `prefix`, `updates` and `played` -- the played Packing -- set.  Its own
    final state is in every episode's tree, so best.score >= best.played.score always.  Tree terminals only, unless playout_incumbents
    is on.  A driver passed in must have been built with record_best=True.
    move_rule=_lib.MOVE_INCUMBENT: every move follows the episode's incumbent where that is followable (it scores above 0 and its line
    passes through the current state), else the first argmax of the visit counts (rp_engine.h: RP_MOVE_INCUMBENT).  The played packing
    then IS the incumbent wherever the incumbent scores above 0, so it works with and without best=True: without it the played packings
    come back, and the driver is still built with record_best=True.  A driver passed in without record_best is a RuntimeError.
    playout_incumbents (with best or move_rule=MOVE_INCUMBENT, and evaluator="rollout"): every random playout the search runs is a candidate too
    (rp_set_incumbent_playouts) -- in a network-free search they are nearly all the finished packings it ever computes; the incumbents
    then carry `tree_moves` and `playout`.  A driver passed in must have been built with the same setting.
    playout_policy (with evaluator="rollout"): how the playouts choose among the legal moves (rp_set_playout_policy) -- "uniform" (the
    default), "area", "width", "width2", "height", "height2", or a pair (w_pow, h_pow): a move of an item (w, h) weighs
    w^w_pow * h^h_pow.  ValueError for anything else and with the network as evaluator.  A driver passed in must have been built
    with the same policy.
    playout_landing (with evaluator="rollout"): the landing power of the playouts (rp_set_playout_landing) -- 0 (the default), 1 or 2: a
    legal move that lands on row t weighs (H - t)^playout_landing times its weight under playout_policy.  ValueError for anything else
    and with the network as evaluator.  A driver passed in must have been built with the same power.
    rollout_prior (with evaluator="rollout"): the prior of the search's leaves (rp_set_rollout_prior) -- "uniform" (the default), "low",
    "low2", "width2", "area", "width2-low2", or a triple (w_pow, h_pow, land_pow): a legal move of an item (w, h) that lands on row t
    weighs w^w_pow * h^h_pow * (H - t)^land_pow.  ValueError for anything else and with the network as evaluator.  A driver passed in
    must have been built with the same prior."""
    from .selfplay import BatchedSelfPlay
    _check_instances(item_wh, seeds, initial_board, remaining)
    policy = _lib.playout_policy_powers(playout_policy)
    if policy != (0, 0) and (_evaluator_of(driver, driver_kw) != "rollout"):
        raise ValueError("a playout policy other than 'uniform' needs evaluator='rollout'")
    landing = _lib.playout_landing_power(playout_landing)
    if landing != 0 and (_evaluator_of(driver, driver_kw) != "rollout"):
        raise ValueError("a playout landing power other than 0 needs evaluator='rollout'")
    prior = _lib.rollout_prior_powers(rollout_prior)
    if prior != (0, 0, 0) and (_evaluator_of(driver, driver_kw) != "rollout"):
        raise ValueError("a rollout prior other than 'uniform' needs evaluator='rollout'")
    n = len(item_wh) if seeds is None else len(seeds)
    rule = greedy_rule(args) if move_rule is None else int(move_rule)
    sp = driver
    follow = rule == _lib.MOVE_INCUMBENT  # the rule plays along the incumbents: the driver keeps them whether they are returned or not
    if playout_incumbents and not (best or follow):
        raise ValueError("playout_incumbents is a property of the incumbents: it needs best=True or move_rule=MOVE_INCUMBENT")
    if follow and sp is not None and not sp.record_best:
        raise RuntimeError("the driver was built without record_best")
    if sp is None:
        games = int(games or min(max(n, 1), 4096))
        driver_kw.setdefault("groups", max(1, min(2, games)))
        sp = BatchedSelfPlay(game, nnet, args, games=games, move_rule=rule, seed=seed, max_examples=0, record_packings=True, record_best=bool(best) or follow,
                             playout_incumbents=bool(playout_incumbents), playout_policy=policy, rollout_prior=prior, playout_landing=landing,
                             **driver_kw)
    elif sp.playout_incumbents != bool(playout_incumbents):
        raise RuntimeError("the driver was built with playout_incumbents=%r" % sp.playout_incumbents)
    elif sp.playout_policy != policy:
        raise RuntimeError("the driver was built with playout_policy=%r" % (sp.playout_policy,))
    elif sp.playout_landing != landing:
        raise RuntimeError("the driver was built with playout_landing=%r" % (sp.playout_landing,))
    elif sp.rollout_prior != prior:
        raise RuntimeError("the driver was built with rollout_prior=%r" % (sp.rollout_prior,))
    elif sp.move_rule != rule:
        sp.set_move_rule(rule)
    try:
        return play_packings(sp, item_wh=item_wh, seeds=seeds, total_area=total_area, bin_h=bin_h, bin_w=bin_w, rewards_list=rewards_list,
                             initial_board=initial_board, remaining=remaining, best=best)
    finally:
        if driver is None:
            sp.close()


def random_scores(game, item_wh=None, seeds=None, playouts=16, seed=0, bin_h=None, bin_w=None, initial_board=None, remaining=None,
                  playout_policy="uniform", playout_landing=0):
    """Scores of random packings -> float64 [n, playouts]: `playouts` random playouts of every instance from the empty bin, or
    from (initial_board, remaining) as pack() takes them
    (rp_rollout_states; instance i plays as episode i, playout j draws from (seed, i, j)).  The random baseline a search or a trained
    network is compared with, and -- flattened -- a first R2 buffer for pack(..., evaluator="rollout", rewards_list=...).
    item_wh / seeds / bin_h / bin_w: the instances, as pack() takes them.  playout_policy: uniform over the legal moves by default, or
    weighted by the item as pack() takes it -- a buffer for a search under a policy wants the scores of that policy.  playout_landing: the
    playouts' landing power, likewise."""
    _check_instances(item_wh, seeds, initial_board, remaining)
    policy = _lib.playout_policy_powers(playout_policy)
    landing = _lib.playout_landing_power(playout_landing)
    W, H, N = game.bin_width, game.bin_height, game.num_items
    rows0 = rem0 = None
    if seeds is None:  # checked before an engine is built
        item_wh, rows0, rem0, area = initial_state(W, H, N, item_wh, initial_board, remaining)
    eng = _lib.Engine(W, H, N, 1, 1, seed=int(seed) & 0x7FFFFFFFFFFFFFFF)
    try:
        if policy != (0, 0):
            eng.set_playout_policy(*policy)
        if landing != 0:
            eng.set_playout_landing(landing)
        if seeds is not None:
            item_wh = eng.generate_items(seeds, bin_w=bin_w, bin_h=bin_h)
            area = np.full(len(item_wh), int(bin_w or W) * int(bin_h or H), np.int32)
        n = len(item_wh)
        if n == 0:
            return np.zeros((0, int(playouts)), np.float64)
        if rows0 is None:
            rows0, rem0 = np.zeros((n, H), np.uint64), np.ones((n, N), np.uint8)
        max_h = (item_wh[:, :, 1] * rem0).max(axis=1).astype(np.int32)  # over the items that take part, as rp_set_instance_initial
        _, score, _, _ = eng.rollout_states(rows0, rem0, item_wh, area, max_h, (), 0.75, playouts,
                                            episode_id=np.arange(n, dtype=np.uint64), boards=False)
        return score
    finally:
        eng.close()
