"""Measurements of the playout policy (rp_set_playout_policy) for profiles/playout_policy.md, on one GPU.

  python scripts/probe_playout_policy.py time [--policy width2] [--lib PATH]
      Time per k_rollout launch (HIP events around rp_rollout_eval), 20x20 / 32 items cut from 20x15 by the device generator, 4 096 slots
      in one group, 8 playouts per leaf -- the slot and playout counts of profiles/rollout_eval.md:
        root:   every slot waits at its root (the empty bin); the same launch is repeated, so every build and every repeat times the
                same playouts of one policy;
        search: the eager waves of a running search (100 simulations per move, auto-restart from a pool of 8 192 seeds, R2 buffer =
                random_scores of the first 256 seeds x 16 playouts under the policy), 60 waves of warm-up, then 1 000 timed waves.
      --lib: time another build of the engine (the parent commit's librp_engine.so) through this package; uniform only.
  python scripts/probe_playout_policy.py quality
      256 seeded instances of the same shape through pack(evaluator="rollout", playouts=8, best=True, playout_incumbents=True), 100
      simulations per move, the buffer random_scores() of the same policy: mean played score, mean incumbent score, and in how many
      episodes a weighted policy beats uniform.

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


def game_args():
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=SIMS, cpuct=1, alpha=0.75, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


def stats(ms):
    ms = np.asarray(ms)
    return dict(mean_ms=round(float(ms.mean()), 5), median_ms=round(float(np.median(ms)), 5), min_ms=round(float(ms.min()), 5), launches=int(ms.size))


def time_root(policy, repeats=5, launches=200):
    """-> one stats dict per repeat: `launches` launches of k_rollout over 4 096 slots that all wait at the empty bin."""
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(W, H, N, SLOTS, SIMS, seed=SEED, tie_salt=77, move_rule=_lib.MOVE_ARGMAX_FIRST, stream=torch.cuda.current_stream().cuda_stream)
    if policy != (0, 0):
        eng.set_playout_policy(*policy)
    wh = eng.generate_items(100 + np.arange(SLOTS), bin_w=W, bin_h=BIN_H)
    eng.begin_episodes(wh, np.full(SLOTS, W * BIN_H, np.int32))
    assert eng.search_step() == SLOTS
    v = torch.zeros(SLOTS, device="cuda")
    out = []
    for rep in range(repeats + 1):  # the first repeat is the warm-up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(launches + 1)]
        ev[0].record()
        for k in range(launches):
            eng.rollout_eval(v.data_ptr(), SLOTS, PLAYOUTS)
            ev[k + 1].record()
        torch.cuda.synchronize()
        if rep:
            out.append(stats([ev[k].elapsed_time(ev[k + 1]) for k in range(launches)]))
    eng.check()
    mean_v = float(v.mean())
    eng.close()
    return out, mean_v


def time_search(policy, warmup=60, waves=1000):
    import torch
    from resource_packing_self_play_amd import _lib, solve
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    game, args = game_args()
    seeds = 100 + np.arange(8192)
    kw = {} if policy == (0, 0) else dict(playout_policy=policy)  # another build of the engine is never asked for a policy
    buf = solve.random_scores(game, seeds=seeds[:256], playouts=16, seed=SEED, bin_h=BIN_H, **kw).reshape(-1)
    sp = BatchedSelfPlay(game, None, args, games=SLOTS, groups=1, move_rule=_lib.MOVE_SAMPLE, seed=SEED, evaluator="rollout", playouts=PLAYOUTS,
                         use_graph=False, **kw)
    sp.start_from_seeds(seeds, buf, bin_h=BIN_H)
    g = sp.groups[0]
    ms, waiting = [], []
    with torch.cuda.stream(g.stream):
        for _ in range(warmup):
            g.wave_eager(None)
        ev = []
        for _ in range(waves):
            n = g.eng.search_step()  # synchronises: the events below bracket the playout kernel alone
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(g.stream)
            g.eng.rollout_eval(g.rollout_v.data_ptr(), g.G, PLAYOUTS)
            b.record(g.stream)
            g.eng.commit_eval(g.uniform_pi.data_ptr(), g.rollout_v.data_ptr())
            ev.append((a, b)); waiting.append(n)
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
    g.eng.check()
    sp.close()
    return dict(stats(ms), leaves_waiting=round(float(np.mean(waiting)), 1))


def quality():
    from resource_packing_self_play_amd import solve
    game, args = game_args()
    seeds = 100 + np.arange(256)
    out, played, best = {}, {}, {}
    for name in ("uniform", "area", "width2"):
        scores = solve.random_scores(game, seeds=seeds, playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=name)
        packs = solve.pack(game, None, args, seeds=seeds, bin_h=BIN_H, evaluator="rollout", playouts=PLAYOUTS, rewards_list=scores.reshape(-1), seed=SEED,
                           best=True, playout_incumbents=True, playout_policy=name)
        played[name] = np.array([p.played.score for p in packs]); best[name] = np.array([p.score for p in packs])
        out[name] = dict(random_mean=round(float(scores.mean()), 4), random_dead_ends=round(float((scores == 0).mean()), 4),
                         played_mean=round(float(played[name].mean()), 4), played_complete=int((played[name] > 0).sum()),
                         incumbent_mean=round(float(best[name].mean()), 4), incumbent_complete=int((best[name] > 0).sum()),
                         incumbent_from_playout=int(sum(p.playout >= 0 for p in packs)))
    for name in ("area", "width2"):
        out[name].update(played_beats_uniform=int((played[name] > played["uniform"]).sum()), played_loses=int((played[name] < played["uniform"]).sum()),
                         incumbent_beats_uniform=int((best[name] > best["uniform"]).sum()), incumbent_loses=int((best[name] < best["uniform"]).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "quality"))
    ap.add_argument("--policy", default="uniform")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    from resource_packing_self_play_amd import _lib
    policy = _lib.playout_policy_powers(a.policy)
    if a.lib:  # a build from before the policy: its symbols are not bound, and it is never asked for one
        if policy != (0, 0):
            raise SystemExit("--lib times the uniform playouts of another build")
        _lib.LIB_PATH = os.path.abspath(a.lib)
        for name in ("rp_set_playout_policy", "rp_playout_policy"):
            _lib._SIGS.pop(name)
    if a.mode == "quality":
        print(json.dumps(dict(mode="quality", slots=256, sims=SIMS, playouts=PLAYOUTS, result=quality())))
        return
    root, mean_v = time_root(policy)
    print(json.dumps(dict(mode="time", label=a.label or a.policy, policy=list(policy), lib=a.lib, root=root, root_mean_v=mean_v, search=time_search(policy))))


if __name__ == "__main__":
    main()
