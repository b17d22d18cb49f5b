#!/usr/bin/env python3
"""Generates tests/golden/coach_fresh.npz: two iterations of the reference's CoachBPP.learn (CoachBPP.py:101-196) from an EMPTY
R2 buffer (main_bpp.py's default start), the second one greedy, captured like make_golden.py's gen_coach(): np.random.seed()
without an argument is ignored after one np.random.seed(start), np.random.choice picks the lowest index of the largest
probability, the `r == bl` tie draws ev.tie_value(state) (TieGame), the evaluator is the hashed table evaluator, nnet.train /
save_checkpoint / wandb.log are recorded no-ops.

The reference appends every episode's score to the buffer before the next episode (:134), so iteration 1's episodes after the
first are ranked against the scores of the ones before; the start value is the first one for which the reference ranks at least
one iteration-1 episode -1 (a batched iteration against the iteration's snapshot -- the empty buffer -- values all of them +1).
Imports the unmodified reference like make_golden.py (build container only; only the data file travels).
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coach_fresh.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets up the reference's import path and the absent third-party stand-ins)

ev = mg.ev
W, H, N, SIMS, SALT, EPS, CAP = 10, 10, 8, 20, 17, 12, 10


def capture(start):
    import wandb
    from CoachBPP import CoachBPP

    class CoachNet:
        def __init__(self, game, args):
            self.game, self.kind, self.salt, self.trained = game, args.table_kind, args.table_salt, []

        def predict(self, state):
            rows, rem, _, _ = ev.pack_state(state)
            return ev.table_eval(self.kind, rows, rem, self.game.getActionSize(), self.salt)

        def train(self, examples):
            self.trained.append(len(examples))

        def save_checkpoint(self, folder, filename):
            pass

    g = mg.TieGame(W, H, N, 1)
    g.tie_salt = SALT
    args = mg.Args(numIters=2, numEps=EPS, iterStepThreshold=1, maxlenOfQueue=200000, numMCTSSims=SIMS, cpuct=1, alpha=0.75, seed=100,
                   numItersForTrainExamplesHistory=50, numScoresForRank=CAP, binH_min=6, binH=10, numItems=N, checkpoint=tempfile.mkdtemp(),
                   table_kind="hashed", table_salt=SALT)
    gen = mg.ItemsGenerator(W, H, N)
    coach = CoachBPP(g, CoachNet(g, args), gen.items_generator(args.seed), W * H, gen, args, saved_rewards_list=[])
    episodes, seeds, logged = [], [], []
    orig_exec, orig_gen = coach.executeEpisode, gen.items_generator

    def rec_exec(greedy=False):
        before = [float(x) for x in coach.rewards_list]
        ex = orig_exec(greedy)
        episodes.append(dict(greedy=bool(greedy), seed=seeds[-1], bin_height=int(gen.bin_height), total_area=int(coach.items_total_area),
                             items=np.array(coach.items_list)[:, :2].astype(np.uint8), before=before, score=float(coach.ep_score), examples=ex))
        return ex

    def rec_gen(seed):
        seeds.append(int(seed))
        return orig_gen(seed)
    coach.executeEpisode, gen.items_generator = rec_exec, rec_gen
    orig_seed, orig_choice, orig_log = np.random.seed, np.random.choice, getattr(wandb, "log", None)

    def fake_seed(seed=None):
        if seed is not None:
            orig_seed(seed)

    def fake_choice(a, size=None, replace=True, p=None):
        idx = int(np.argmax(np.asarray(p))) if p is not None else 0
        return idx if isinstance(a, (int, np.integer)) else np.asarray(a).reshape(-1)[idx]
    wandb.log = lambda d, step=None: logged.append((int(step), {k: float(v) for k, v in d.items()}))
    np.random.seed(start)
    np.random.seed, np.random.choice = fake_seed, fake_choice
    try:
        coach.learn()
    finally:
        np.random.seed, np.random.choice = orig_seed, orig_choice
        if orig_log is not None:
            wandb.log = orig_log
    assert len(episodes) == 2 * EPS and len(coach.rewards_list) <= CAP
    return coach, episodes, logged


def main():
    for start in range(1, 200):
        coach, episodes, logged = capture(start)
        if any(int(r) == -1 for e in episodes[:EPS] for _, _, r in e["examples"]):
            break
    else:
        raise RuntimeError("no start value ranks an iteration-1 episode -1")
    ex_ep, ex_rows, ex_rem, ex_pi, ex_r = [], [], [], [], []
    for k, e in enumerate(episodes):
        for state, pi, r in e["examples"]:
            rows, rem, _, _ = ev.pack_state(state)
            ex_ep.append(k); ex_rows.append(rows); ex_rem.append(rem); ex_pi.append(np.asarray(pi, np.float64)); ex_r.append(int(r))
    blen = max(len(e["before"]) for e in episodes)
    before = np.full((len(episodes), blen), np.nan)
    for k, e in enumerate(episodes):
        before[k, :len(e["before"])] = e["before"]
    metrics = {}
    for step, dd in logged:
        metrics.setdefault(step, {}).update(dd)
    meta = dict(mg.META, generator="tests/golden/make_coach_fresh.py")
    np.savez_compressed(os.path.join(HERE, "coach_fresh.npz"), meta=json.dumps(meta), start=start, W=W, H=H, N=N, sims=SIMS, salt=SALT, kind="hashed",
                        alpha=0.75, numEps=EPS, numIters=2, iterStepThreshold=1, numScoresForRank=CAP, binH_min=6, binH=10, initial=np.zeros(0),
                        ep_seed=np.array([e["seed"] for e in episodes], np.int64), ep_bin_height=np.array([e["bin_height"] for e in episodes], np.int32),
                        ep_area=np.array([e["total_area"] for e in episodes], np.int32), ep_items=np.stack([e["items"] for e in episodes]),
                        ep_greedy=np.array([e["greedy"] for e in episodes]), ep_score=np.array([e["score"] for e in episodes]), ep_before=before,
                        ep_before_len=np.array([len(e["before"]) for e in episodes], np.int32), after_iter1=np.array(episodes[EPS]["before"]),
                        after_iter2=np.array([float(x) for x in coach.rewards_list]), ex_ep=np.array(ex_ep, np.int32), ex_rows=np.stack(ex_rows),
                        ex_rem=np.stack(ex_rem), ex_pi=np.stack(ex_pi), ex_r=np.array(ex_r, np.int8), trained_on=np.array(coach.nnet.trained, np.int64),
                        metrics=json.dumps(metrics))
    for it in range(2):
        eps = episodes[it * EPS:(it + 1) * EPS]
        print("iteration %d: bin_height %d, scores %s, r %s" % (it + 1, eps[0]["bin_height"], [round(e["score"], 4) for e in eps],
                                                               [int(e["examples"][0][2]) for e in eps]))
    print("wrote coach_fresh.npz (start %d)" % start)


if __name__ == "__main__":
    main()
