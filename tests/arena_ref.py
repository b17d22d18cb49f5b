"""Host model of the engine's level arena, written from the `Arena` comment in rp_engine.hip alone (test infrastructure).

The arena hands out runs of entries by bump allocation in fixed-size chunks, one open chunk per game level (level = items placed).
A run never spans two chunks.  A level that needs room takes the most recently recycled chunk, else the next chunk that was never
used; when a level dies its chunks go back on the stack of recycled ones.  The model predicts where a run lands (the offsets that
rp_dump_tree exports as node_edge_off), how many chunks an episode needs (what rp_arena_peak reports and what edge_cap / vis_cap
have to provide) and when a reservation fails.  Nothing here looks at the engine's outputs.
"""


class LevelArena:
    def __init__(self, chunk, n_chunks):
        if chunk < 1 or n_chunks < 0:
            raise ValueError("chunk >= 1 and n_chunks >= 0")
        self.chunk, self.n_chunks = int(chunk), int(n_chunks)
        self._peak = 0
        self.fresh = 0
        self.reset()

    def reset(self):
        """A new episode: no level has a chunk, nothing is recycled, every chunk counts as never used again.  The high-water mark
        survives (it is one over all episodes)."""
        self._peak = max(self._peak, self.fresh)
        self.open = {}     # level -> chunk being filled
        self.used = {}     # level -> entries taken in that chunk
        self.chunks = {}   # level -> the level's chunks, newest (head) first
        self.stack = []    # recycled chunks, top last
        self.fresh = 0     # never-used chunks taken so far

    @property
    def peak(self):
        """High-water mark of never-used chunks taken: a never-used chunk is taken only while nothing is recycled, so this is also
        the largest number of chunks ever in use."""
        return max(self._peak, self.fresh)

    def reserve(self, level, need):
        """Offset of a run of `need` entries at `level`, or None when the arena is exhausted (the state is then unchanged)."""
        need = int(need)
        if need < 1 or need > self.chunk:
            raise ValueError("a run has 1 .. chunk entries (got %d, chunk %d)" % (need, self.chunk))
        c = self.open.get(level)
        if c is None or self.used[level] + need > self.chunk:
            if self.stack:
                c = self.stack.pop()
            elif self.fresh < self.n_chunks:
                c = self.fresh
                self.fresh += 1
            else:
                return None
            self.chunks.setdefault(level, []).insert(0, c)
            self.open[level] = c
            self.used[level] = 0
        off = c * self.chunk + self.used[level]
        self.used[level] += need
        return off

    def free_level(self, level):
        """The level is dead: its chunks go onto the stack, head (newest) first, so its oldest chunk is reused first."""
        self.stack.extend(self.chunks.pop(level, []))
        self.open.pop(level, None)
        self.used.pop(level, None)


UNLIMITED = 0xFFFE  # the engine's chunk ids are 16 bits wide


def tree_nodes(dump, n_valid_of):
    """Oracle dump() (a dict in creation order: the oracle appends a node at a state's first sight and dump walks them by index) ->
    list of (level, n_valid, vis_n) per node.  level = items placed; a terminal node has no legal move; an expanded node carries its
    legal moves, for a node that was created but never expanded n_valid_of(rows bytes, rem bytes) has to count them.  vis_n = the
    legal moves with a visit."""
    out = []
    for (rows, rem), rec in dump.items():
        level = sum(1 for b in rem if b == 0)
        if rec["es"] != 0:
            out.append((level, 0, 0))
        elif rec["expanded"]:
            out.append((level, len(rec["actions"]), int(sum(1 for n in rec["nsa"] if n > 0))))
        else:
            out.append((level, int(n_valid_of(rows, rem)), 0))
    return out


def prior_layout(nodes, pchunk, moves=None, root_level=0, n_chunks=UNLIMITED):
    """Where the legal-move runs of an episode's nodes land.  nodes: (level, n_valid[, ...]) in creation order; a terminal node
    (n_valid 0) reserves nothing.  moves: with reclaim, the node counts at which a move was played -- move j kills level
    root_level + j after moves[j] nodes exist (a node the move itself creates is counted before it).  -> (offset per node, None for
    a terminal one or once the arena is exhausted; chunks the episode needs = the arena's peak)."""
    arena = LevelArena(pchunk, n_chunks)
    moves = list(moves or [])
    offs, j, full = [], 0, False
    for i, nd in enumerate(nodes):
        while j < len(moves) and moves[j] <= i:
            arena.free_level(root_level + j)
            j += 1
        level, n_valid = nd[0], nd[1]
        off = None
        if n_valid > 0 and not full:
            off = arena.reserve(level, n_valid)
            full = off is None
        offs.append(off)
    return offs, arena.peak


def visited_consumed(n_valid, vis_n):
    """Entries of the visited arena a node has taken and its largest block: the block grows 2, 4, 8, ... capped at n_valid, every
    growth takes a new block and abandons the old one."""
    if vis_n == 0:
        return 0, 0
    cap = min(2, n_valid)
    total = cap
    while cap < vis_n:
        cap = min(2 * cap, n_valid)
        total += cap
    return total, cap


def visited_bounds(nodes, vchunk):
    """(lower, upper) bound of the chunks the visited arena opens for a tree without reclaim.  nodes: (level, n_valid, vis_n).  A level
    that consumed S entries in blocks of at most b entries opened at least ceil(S / vchunk) chunks and -- a chunk is left only when a
    block of <= b entries does not fit, i.e. with more than vchunk - b entries taken -- at most ceil(S / (vchunk - b + 1)).  How the
    blocks pack in between depends on the order of growth, which a finished tree does not tell."""
    per = {}
    for level, n_valid, vis_n in nodes:
        s, b = visited_consumed(n_valid, vis_n)
        if s:
            S, B = per.get(level, (0, 0))
            per[level] = (S + s, max(B, b))
    lo = sum(-(-S // vchunk) for S, B in per.values())
    hi = sum(-(-S // (vchunk - B + 1)) for S, B in per.values())
    return lo, hi
