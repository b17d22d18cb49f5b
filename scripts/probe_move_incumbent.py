"""Measurements of the move rule that follows the incumbent (RP_MOVE_INCUMBENT) for profiles/move_incumbent.md, on one GPU.

  python scripts/probe_move_incumbent.py quality
      The 256 instances and settings of profiles/playout_landing.md -- 20x20 / 32 items cut from 20x15 by the device generator, 100
      simulations per move, 8 playouts, playout incumbents on, the buffer random_scores() of the same policy -- through
      pack(evaluator="rollout", best=True, playout_incumbents=True) under width2 and under area + landing 2, each under the uniform
      prior and under low2, once with RP_MOVE_ARGMAX_FIRST and once with RP_MOVE_INCUMBENT: mean played score, complete played
      episodes, mean incumbent score, episodes played / incumbent better and worse than under RP_MOVE_ARGMAX_FIRST, the share of moves
      that followed the incumbent (counter [14] over counter [8]), wall time of the one pack() call, and whether the invariant held
      (played == incumbent wherever the incumbent scores above 0).
  python scripts/probe_move_incumbent.py moves [--rule incumbent|argmax_first]
      Time of k_moves per launch from HIP events.  The kernel is launched inside rp_search_step together with k_search and k_incumbent,
      so the launch is isolated: 4 096 slots of the same shape (width2 playouts, playout incumbents, 16 simulations per move) run
      under RP_MOVE_EXTERNAL, where rp_search_step launches no k_moves and the slots wait as MOVE_READY; the first 8 moves are played by
      the host with the rule itself (rp_incumbents, rp_root_counts, rp_advance_roots), so that every incumbent's line passes through
      the root.  At move 8, with every slot MOVE_READY: five timed rp_search_step calls without k_moves (k_search and k_incumbent
      return at once), then the rule is set with rp_set_sims(0) and one rp_search_step is timed -- k_moves plays a move in all 4 096
      slots, k_search only flips them back to MOVE_READY.  10 such repeats after a warm-up; reported: both step times and the median
      difference, the time of the k_moves launch.

Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, BIN_H, N = 20, 20, 15, 32
PLAYOUTS, SIMS = 8, 100
SEED = 20251
SETTINGS = (("width2", 0), ("area", 2))
PRIORS = ("uniform", "low2")


def game_args(sims=SIMS):
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame
    from resource_packing_self_play_amd.utils import dotdict
    return BinPackingGame(W, H, N, 1), dotdict(numMCTSSims=sims, cpuct=1, alpha=0.75, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8)


def quality():
    from resource_packing_self_play_amd import _lib, solve
    from resource_packing_self_play_amd.selfplay import BatchedSelfPlay
    game, args = game_args()
    seeds = 100 + np.arange(256)
    out = {}
    for prior in PRIORS:
        for policy, landing in SETTINGS:
            buf = solve.random_scores(game, seeds=seeds, playouts=16, seed=SEED, bin_h=BIN_H, playout_policy=policy, playout_landing=landing).reshape(-1)
            base = None
            for name, rule in (("argmax_first", _lib.MOVE_ARGMAX_FIRST), ("incumbent", _lib.MOVE_INCUMBENT)):
                key = "%s+%d/%s/%s" % (policy, landing, prior, name)
                # the driver pack() would build, built here so that its counters can be read
                sp = BatchedSelfPlay(game, None, args, games=256, move_rule=rule, seed=SEED, max_examples=0, record_packings=True, record_best=True,
                                     playout_incumbents=True, playout_policy=policy, rollout_prior=prior, playout_landing=landing, evaluator="rollout",
                                     playouts=PLAYOUTS, groups=2)
                t = time.perf_counter()
                packs = solve.pack(game, None, args, seeds=seeds, bin_h=BIN_H, rewards_list=buf, move_rule=rule, best=True, playout_incumbents=True,
                                   playout_policy=policy, playout_landing=landing, rollout_prior=prior, driver=sp)
                dt = time.perf_counter() - t
                cnt = sp.counters()
                sp.close()
                played, best = np.array([p.played.score for p in packs]), np.array([p.score for p in packs])
                same = [p.actions.tolist() == p.played.actions.tolist() and p.score == p.played.score for p in packs if p.score > 0]
                out[key] = dict(played_mean=round(float(played.mean()), 4), played_complete=int((played > 0).sum()), incumbent_mean=round(float(best.mean()), 4),
                                incumbent_complete=int((best > 0).sum()), followed_share=round(cnt["followed_moves"] / max(cnt["moves"], 1), 4),
                                played_is_incumbent=int(sum(same)), incumbents_above_0=len(same), wall_s=round(dt, 2))
                if base is None:
                    base = (played, best)
                else:
                    out[key].update(played_better=int((played > base[0]).sum()), played_worse=int((played < base[0]).sum()),
                                    incumbent_better=int((best > base[1]).sum()), incumbent_worse=int((best < base[1]).sum()))
                print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    return out


def moves(rule_name, depth=8, repeats=10, slots=4096, sims=16):
    """Time of one k_moves launch in which every slot plays a move, from HIP events around rp_search_step (module docstring)."""
    import torch
    from resource_packing_self_play_amd import _lib
    rule = _lib.MOVE_INCUMBENT if rule_name == "incumbent" else _lib.MOVE_ARGMAX_FIRST
    eng = _lib.Engine(W, H, N, slots, sims, seed=SEED, tie_salt=77, move_rule=_lib.MOVE_EXTERNAL, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_rank_buffer(np.linspace(0.5, 1.0, 64))
    eng.set_incumbent(True)
    eng.set_incumbent_playouts(True)
    eng.set_playout_policy(2, 0)
    wh = eng.generate_items(100 + np.arange(slots), bin_w=W, bin_h=BIN_H)
    pi = torch.zeros((slots, eng.A), device="cuda"); v = torch.zeros(slots, device="cuda")

    def timed_step():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); eng.search_step(sync=False); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    with_moves, without, played, followed = [], [], 0, 0
    for rep in range(repeats + 1):  # the first repeat is the warm-up
        eng.set_move_rule(_lib.MOVE_EXTERNAL)
        eng.set_sims(sims)
        eng.begin_episodes(wh, np.full(slots, W * BIN_H, np.int32))
        for m in range(depth + 1):
            while True:  # search until every slot has spent its budget: without k_moves they all wait as MOVE_READY
                if eng.search_step():
                    eng.rollout_eval(v.data_ptr(), slots, PLAYOUTS, pi_ptr=pi.data_ptr())
                    eng.commit_eval(pi.data_ptr(), v.data_ptr())
                elif (eng.status()[0] == _lib.PHASE_MOVE_READY).all():
                    break
            if m < depth:  # the rule applied on the host, so that every incumbent's line passes through the root at the timed move
                inc, counts = eng.incumbents(), eng.root_counts()
                follow = (inc["score"] > 0) & (inc["moves"] > m)
                ended, _ = eng.advance_roots(np.where(follow, inc["action"][:, m], counts.argmax(axis=1)))
                assert not ended.any()
        base = [timed_step() for _ in range(5)]  # RP_MOVE_EXTERNAL: no k_moves, k_search and k_incumbent return at once
        eng.set_move_rule(rule)
        eng.set_sims(0)  # k_search flips the slots back to MOVE_READY without a simulation: the step is k_moves and two empty launches
        eng.counters(reset=True)
        t = timed_step()
        cnt = eng.counters()
        assert cnt["moves"] == slots and cnt["simulations"] == 0
        if rep:
            with_moves.append(t); without.append(float(np.median(base))); played += cnt["moves"]; followed += cnt["followed_moves"]
    eng.check()
    eng.close()
    a, b = np.array(with_moves), np.array(without)
    return dict(rule=rule_name, slots=slots, move=depth, repeats=repeats, followed_share=round(followed / played, 4),
                step_ms=dict(median=round(float(np.median(a)), 5), min=round(float(a.min()), 5), max=round(float(a.max()), 5)),
                step_without_k_moves_ms=dict(median=round(float(np.median(b)), 5), min=round(float(b.min()), 5), max=round(float(b.max()), 5)),
                k_moves_ms_median=round(float(np.median(a - b)), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("quality", "moves"))
    ap.add_argument("--rule", default="incumbent", choices=("incumbent", "argmax_first"))
    a = ap.parse_args()
    if a.mode == "quality":
        print(json.dumps(dict(mode="quality", instances=256, sims=SIMS, playouts=PLAYOUTS, result=quality())))
    else:
        print(json.dumps(dict(mode="moves", result=moves(a.rule))))


if __name__ == "__main__":
    main()
