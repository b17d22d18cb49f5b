"""Measurements of the rollout prior (rp_set_rollout_prior) for profiles/rollout_prior.md, on one GPU.

  python scripts/probe_rollout_prior.py time [--prior width2-low2] [--lib PATH]
      Time per rp_rollout_eval call (HIP events around it: k_rollout, and k_rollout_prior under a prior), 20x20 / 32 items cut from
      20x15 by the device generator, 4 096 slots in one group, 8 playouts per leaf under the playout policy width2 -- the shape of
      profiles/playout_policy.md:
        root:   every slot waits at its root (the empty bin); the same call is repeated, a warm-up repeat and then 5 timed ones of 200
                calls each;
        search: the eager waves of a running search (100 simulations per move, auto-restart from a pool of 8 192 seeds, R2 buffer =
                random_scores of the first 256 seeds x 16 playouts under width2), 60 waves of warm-up, then 5 repeats of 200 timed waves.
      --lib: time another build of the engine (the parent commit's librp_engine.so) through this package; uniform prior only.
  python scripts/probe_rollout_prior.py quality
      256 seeded instances of the same shape through pack(evaluator="rollout", playouts=8, best=True, playout_incumbents=True,
      playout_policy="width2"), 100 simulations per move, the buffer random_scores() under width2, under the priors uniform, width2,
      low2 and width2-low2: mean played score, mean incumbent score, complete packings, and in how many episodes a prior beats or
      loses to the uniform one.

Each mode prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, BIN_H, N = 20, 20, 15, 32
SLOTS, PLAYOUTS, SIMS = 4096, 8, 100
SEED = 20251
POLICY = "width2"
PRIORS = ("uniform", "width2", "low2", "width2-low2")
NEW_SYMBOLS = ("rp_set_rollout_prior", "rp_rollout_prior", "rp_rollout_prior_states")


def game_args():
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=SIMS, cpuct=1, alpha=0.75, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


def stats(ms):
    ms = np.asarray(ms)
    return dict(mean_ms=round(float(ms.mean()), 5), median_ms=round(float(np.median(ms)), 5), min_ms=round(float(ms.min()), 5), calls=int(ms.size))


def time_root(prior, repeats=5, calls=200):
    """-> one stats dict per repeat: `calls` calls of rp_rollout_eval over 4 096 slots that all wait at the empty bin."""
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, SLOTS, SIMS, seed=SEED, tie_salt=77, move_rule=_lib.MOVE_ARGMAX_FIRST, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_playout_policy(*_lib.playout_policy_powers(POLICY))
    pi = None
    if prior != (0, 0, 0):
        eng.set_rollout_prior(*prior)
        pi = torch.zeros((SLOTS, W * N), device="cuda")
    wh = eng.generate_items(100 + np.arange(SLOTS), bin_w=W, bin_h=BIN_H)
    eng.begin_episodes(wh, np.full(SLOTS, W * BIN_H, np.int32))
    assert eng.search_step() == SLOTS
    v = torch.zeros(SLOTS, device="cuda")
    out = []
    for rep in range(repeats + 1):  # the first repeat is the warm-up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
        ev[0].record()
        for k in range(calls):
            eng.rollout_eval(v.data_ptr(), SLOTS, PLAYOUTS, pi_ptr=pi.data_ptr() if pi is not None else None)
            ev[k + 1].record()
        torch.cuda.synchronize()
        if rep:
            out.append(stats([ev[k].elapsed_time(ev[k + 1]) for k in range(calls)]))
    eng.check()
    mean_v = float(v.mean())
    eng.close()
    return out, mean_v


def time_search(prior, warmup=60, repeats=5, waves=200):
    import torch
    from resource_packing_self_play_amd import _lib, solve
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    game, args = game_args()
    seeds = 100 + np.arange(8192)
    kw = {} if prior == (0, 0, 0) else dict(rollout_prior=prior)  # another build of the engine is never asked for a prior
    buf = solve.random_scores(game, seeds=seeds[:256], playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=POLICY).reshape(-1)
    sp = BatchedSelfPlay(game, None, args, games=SLOTS, groups=1, move_rule=_lib.MOVE_SAMPLE, seed=SEED, evaluator="rollout", playouts=PLAYOUTS,
                         use_graph=False, playout_policy=POLICY, **kw)
    sp.start_from_seeds(seeds, buf, bin_h=BIN_H)
    g = sp.groups[0]
    pi = g.uniform_pi if prior == (0, 0, 0) else g.prior_pi
    out, waiting = [], []
    with torch.cuda.stream(g.stream):
        for _ in range(warmup):
            g.wave_eager(None)
        for _ in range(repeats):
            ev = []
            for _ in range(waves):
                n = g.eng.search_step()  # synchronises: the events below bracket rp_rollout_eval alone
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(g.stream)
                g.eng.rollout_eval(g.rollout_v.data_ptr(), g.G, PLAYOUTS, pi_ptr=None if prior == (0, 0, 0) else pi.data_ptr())
                b.record(g.stream)
                g.eng.commit_eval(pi.data_ptr(), g.rollout_v.data_ptr())
                ev.append((a, b)); waiting.append(n)
            torch.cuda.synchronize()
            out.append(stats([a.elapsed_time(b) for a, b in ev]))
    g.eng.check()
    sp.close()
    return out, round(float(np.mean(waiting)), 1)


def quality():
    from resource_packing_self_play_amd import solve
    game, args = game_args()
    seeds = 100 + np.arange(256)
    scores = solve.random_scores(game, seeds=seeds, playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=POLICY)
    out, played, best = {}, {}, {}
    for name in PRIORS:
        packs = solve.pack(game, None, args, seeds=seeds, bin_h=BIN_H, evaluator="rollout", playouts=PLAYOUTS, rewards_list=scores.reshape(-1), seed=SEED,
                           best=True, playout_incumbents=True, playout_policy=POLICY, rollout_prior=name)
        played[name] = np.array([p.played.score for p in packs]); best[name] = np.array([p.score for p in packs])
        out[name] = dict(played_mean=round(float(played[name].mean()), 4), played_complete=int((played[name] > 0).sum()),
                         incumbent_mean=round(float(best[name].mean()), 4), incumbent_complete=int((best[name] > 0).sum()),
                         incumbent_from_playout=int(sum(p.playout >= 0 for p in packs)))
    for name in PRIORS[1:]:
        out[name].update(played_beats_uniform=int((played[name] > played["uniform"]).sum()), played_loses=int((played[name] < played["uniform"]).sum()),
                         incumbent_beats_uniform=int((best[name] > best["uniform"]).sum()), incumbent_loses=int((best[name] < best["uniform"]).sum()))
    return dict(random_mean=round(float(scores.mean()), 4), priors=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "quality"))
    ap.add_argument("--prior", default="uniform")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    from resource_packing_self_play_amd import _lib
    prior = _lib.rollout_prior_powers(a.prior)
    if a.lib:  # a build from before the prior: its symbols are not bound, and it is never asked for one
        if prior != (0, 0, 0):
            raise SystemExit("--lib times the uniform prior of another build")
        _lib.LIB_PATH = os.path.abspath(a.lib)
        for name in NEW_SYMBOLS:
            _lib._SIGS.pop(name)
    if a.mode == "quality":
        print(json.dumps(dict(mode="quality", instances=256, sims=SIMS, playouts=PLAYOUTS, playout_policy=POLICY, result=quality())))
        return
    root, mean_v = time_root(prior)
    search, waiting = time_search(prior)
    print(json.dumps(dict(mode="time", label=a.label or a.prior, prior=list(prior), lib=a.lib, root=root, root_mean_v=mean_v, search=search,
                          leaves_waiting=waiting)))


if __name__ == "__main__":
    main()
