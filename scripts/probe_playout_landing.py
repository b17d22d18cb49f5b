"""Measurements of the playouts' landing power (rp_set_playout_landing) for profiles/playout_landing.md, on one GPU.

  python scripts/probe_playout_landing.py time [--policy width2] [--landing 2] [--lib PATH] [--label NAME]
      Time per rp_rollout_eval call (HIP events around it: k_rollout), 20x20 / 32 items cut from 20x15 by the device generator, 4 096
      slots in one group that all wait at their root (the empty bin), 8 playouts per leaf: the same call is repeated, a warm-up repeat
      and then 5 timed ones of 200 calls each.
      --lib: time another build of the engine (the parent commit's librp_engine.so) through this package; landing 0 only.
  python scripts/probe_playout_landing.py scores
      random_scores() of 256 seeded instances of the same shape x 16 playouts under uniform, width2, width2 + landing 1 / 2 and area +
      landing 2: wall time of the call, mean score and the share of dead ends (score 0).
  python scripts/probe_playout_landing.py quality
      The 256 instances through pack(evaluator="rollout", playouts=8, best=True, playout_incumbents=True), 100 simulations per move, the
      buffer random_scores() of the same setting, under width2, width2 + landing 2 and area + landing 2, each under the uniform prior
      and under low2: mean played score, complete packings, mean incumbent score, better / worse counts against width2 under the same
      prior, wall time of the call.

Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, BIN_H, N = 20, 20, 15, 32
SLOTS, PLAYOUTS, SIMS = 4096, 8, 100
SEED = 20251
NEW_SYMBOLS = ("rp_set_playout_landing", "rp_playout_landing")
SCORE_SETTINGS = (("uniform", 0), ("width2", 0), ("width2", 1), ("width2", 2), ("area", 2))
QUALITY_SETTINGS = (("width2", 0), ("width2", 2), ("area", 2))
QUALITY_PRIORS = ("uniform", "low2")


def game_args():
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=SIMS, cpuct=1, alpha=0.75, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


def stats(ms):
    ms = np.asarray(ms)
    return dict(mean_ms=round(float(ms.mean()), 5), median_ms=round(float(np.median(ms)), 5), min_ms=round(float(ms.min()), 5), calls=int(ms.size))


def time_root(policy, landing, repeats=5, calls=200):
    """-> one stats dict per repeat: `calls` calls of rp_rollout_eval over 4 096 slots that all wait at the empty bin."""
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, SLOTS, SIMS, seed=SEED, tie_salt=77, move_rule=_lib.MOVE_ARGMAX_FIRST, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_playout_policy(*policy)
    if landing:
        eng.set_playout_landing(landing)
    wh = eng.generate_items(100 + np.arange(SLOTS), bin_w=W, bin_h=BIN_H)
    eng.begin_episodes(wh, np.full(SLOTS, W * BIN_H, np.int32))
    assert eng.search_step() == SLOTS
    v = torch.zeros(SLOTS, device="cuda")
    out = []
    for rep in range(repeats + 1):  # the first repeat is the warm-up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
        ev[0].record()
        for k in range(calls):
            eng.rollout_eval(v.data_ptr(), SLOTS, PLAYOUTS)
            ev[k + 1].record()
        torch.cuda.synchronize()
        if rep:
            out.append(stats([ev[k].elapsed_time(ev[k + 1]) for k in range(calls)]))
    eng.check()
    mean_v = float(v.mean())
    eng.close()
    return out, mean_v


def scores():
    import torch
    from resource_packing_self_play_amd import solve
    game, _ = game_args()
    seeds = 100 + np.arange(256)
    out = {}
    for policy, landing in SCORE_SETTINGS:
        best = None
        for _ in range(3):  # the first call carries the process's start-up
            torch.cuda.synchronize(); t = time.perf_counter()
            r = solve.random_scores(game, seeds=seeds, playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=policy, playout_landing=landing)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        out["%s+%d" % (policy, landing)] = dict(mean=round(float(r.mean()), 4), dead_end_share=round(float((r == 0).mean()), 4), wall_s=round(best, 4))
    return out


def quality():
    from resource_packing_self_play_amd import solve
    game, args = game_args()
    seeds = 100 + np.arange(256)
    out = {}
    for prior in QUALITY_PRIORS:
        played, best = {}, {}
        for policy, landing in QUALITY_SETTINGS:
            key = "%s+%d/%s" % (policy, landing, prior)
            buf = solve.random_scores(game, seeds=seeds, playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=policy, playout_landing=landing).reshape(-1)
            t = time.perf_counter()
            packs = solve.pack(game, None, args, seeds=seeds, bin_h=BIN_H, evaluator="rollout", playouts=PLAYOUTS, rewards_list=buf, seed=SEED, best=True,
                               playout_incumbents=True, playout_policy=policy, playout_landing=landing, rollout_prior=prior)
            dt = time.perf_counter() - t
            played[key] = np.array([p.played.score for p in packs]); best[key] = np.array([p.score for p in packs])
            out[key] = dict(buffer_mean=round(float(buf.mean()), 4), played_mean=round(float(played[key].mean()), 4), played_complete=int((played[key] > 0).sum()),
                            incumbent_mean=round(float(best[key].mean()), 4), incumbent_complete=int((best[key] > 0).sum()),
                            incumbent_from_playout=int(sum(p.playout >= 0 for p in packs)), wall_s=round(dt, 2))
            base = "width2+0/%s" % prior
            if key != base:
                out[key].update(played_better=int((played[key] > played[base]).sum()), played_worse=int((played[key] < played[base]).sum()),
                                incumbent_better=int((best[key] > best[base]).sum()), incumbent_worse=int((best[key] < best[base]).sum()))
            print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "scores", "quality"))
    ap.add_argument("--policy", default="uniform")
    ap.add_argument("--landing", type=int, default=0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    from resource_packing_self_play_amd import _lib
    if a.lib:  # a build from before the landing power: its symbols are not bound, and it is never asked for one
        if a.landing:
            raise SystemExit("--lib times landing 0 of another build")
        _lib.LIB_PATH = os.path.abspath(a.lib)
        for name in NEW_SYMBOLS:
            _lib._SIGS.pop(name)
    if a.mode == "scores":
        print(json.dumps(dict(mode="scores", instances=256, playouts=16, result=scores())))
    elif a.mode == "quality":
        print(json.dumps(dict(mode="quality", instances=256, sims=SIMS, playouts=PLAYOUTS, result=quality())))
    else:
        policy = _lib.playout_policy_powers(a.policy)
        root, mean_v = time_root(policy, _lib.playout_landing_power(a.landing))
        print(json.dumps(dict(mode="time", label=a.label or "%s+%d" % (a.policy, a.landing), lib=a.lib, root=root, root_mean_v=mean_v)))


if __name__ == "__main__":
    main()
