"""Python restatement of an episode that starts from an arbitrary state (include/rp_engine.h: rp_set_instance_initial) over the
oracle's own functions.  Test infrastructure: the oracle's orc_play_episode always starts from the empty bin with all items, so the
loop of CoachBPP.executeEpisode (CoachBPP.py:70-99) is restated here around OracleMCTS.action_counts, with the oracle's move pick.

Items that do not take part are handed to the oracle with w = h = 0: they have no legal move (their remaining flag is 0) and do not
count in its max_h, which is then the largest h of the items that take part -- the engine's default.  Another max_h (an episode
continued from a prefix, whose placed items count) is lent to the oracle by one absent item of that height.
"""
import numpy as np

import evaluators as ev
import oracle_lib as orc
from rollout_ref import ALPHA, TIE, umulhi

ARGMAX_FIRST, SAMPLE = 0, 1  # orc_play_episode's policies: RP_MOVE_ARGMAX_FIRST / RP_MOVE_SAMPLE


def default_max_h(wh, rem):
    """Largest h among the items that take part, 0 if none (getInitItems, BinPackingGame.py:48, over those items)."""
    h = np.asarray(wh)[:, 1].astype(np.int64) * (np.asarray(rem) != 0)
    return int(h.max()) if len(h) else 0


def begin(m, wh, rem, area, buf, tie_salt, max_h=None):
    """begin_episode of OracleMCTS `m` (built with rollout_ref.ALPHA) for an episode of the items `rem` marks; records on `m` what
    play_from needs."""
    wh = np.asarray(wh, np.uint8)
    present = np.asarray(rem) != 0
    iw, ih = wh[:, 0] * present, wh[:, 1] * present
    own = default_max_h(wh, rem)
    if max_h is not None and int(max_h) != own:
        absent = np.flatnonzero(~present)
        assert int(max_h) > own and len(absent), "the oracle takes max_h from its items: only a larger one, lent to an absent item"
        ih = ih.copy(); ih[absent[0]] = int(max_h)
        own = int(max_h)
    m.begin_episode(iw, ih, area, buf)
    m.episode = dict(iw=iw.astype(np.uint8), ih=ih.astype(np.uint8), area=int(area), max_h=own, buf=list(buf), tie_salt=int(tie_salt))
    return m


def ended(m, board, rem):
    """getGameEnded of a state without a legal move -> (outcome +-1 with the tie drawn from the state, score r)."""
    e = m.episode
    out, r = orc.ranked_reward(m.W, m.H, board, e["area"], e["max_h"], e["buf"], ALPHA)
    if out == TIE:
        out = ev.tie_value(ev.pack_board(board), rem, e["tie_salt"])
    return int(out), float(r)


def play_from(m, board, rem, sims, policy, seed, episode_id):
    """Plays the episode of `m` (after begin()) from (board [H, W] cells, rem [N]) -> dict(actions int32 [moves], rows uint64 [moves]
    (mask of the bin rows each move filled), outcome, score, moves, board uint64 [H] (final bin)).  Moves are numbered from 0 at the
    given state.  A state without a legal move: 0 moves, outcome and score of that state."""
    W, H, N, e = m.W, m.H, m.N, m.episode
    board = np.array(board, np.uint8).reshape(H, W).copy(); rem = (np.asarray(rem) != 0).astype(np.uint8)
    actions, rows = [], []
    outcome = score = None
    if not orc.has_valid_moves(W, H, N, board, e["iw"], e["ih"], rem):
        outcome, score = ended(m, board, rem)
    while outcome is None:
        counts = m.action_counts(board, rem, sims)
        if policy == ARGMAX_FIRST:
            action = int(np.argmax(counts))  # lowest index among the maxima
            assert counts[action] > 0
        else:
            total = int(counts.sum(dtype=np.uint64))
            r = umulhi(orc.lib().orc_sample_u64(int(seed), int(episode_id), len(actions)), total)
            action = int(np.searchsorted(np.cumsum(counts.astype(np.uint64)), r, side="right"))  # first a with cumulative count > r
        rc, after, rem = orc.next_state(W, H, N, board, e["iw"], e["ih"], rem, action)
        assert rc == 0
        changed = (after != board).any(axis=1)
        rows.append(sum(1 << int(r) for r in np.flatnonzero(changed)))
        actions.append(action)
        board = after
        if not orc.has_valid_moves(W, H, N, board, e["iw"], e["ih"], rem):
            outcome, score = ended(m, board, rem)
    return dict(actions=np.array(actions, np.int32), rows=np.array(rows, np.uint64), outcome=outcome, score=score, moves=len(actions),
                board=ev.pack_board(board))
