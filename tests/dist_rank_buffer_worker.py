"""One rank of tests/test_gpu_rank_buffer.py::test_two_ranks_repair_like_one (launched with the torchrun environment): two learn()
iterations in args.rank_buffer = "sequential" mode from an empty buffer, the second greedy with drawn ties.
usage: dist_rank_buffer_worker.py <out dir> <world>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main(out_dir, world):
    import torch
    from engine_util import host_evaluator
    from resource_packing_self_play_amd import distributed as rdist
    from resource_packing_self_play_amd.CoachBPP import CoachBPP
    from resource_packing_self_play_amd.binpacking.BinPackingGame import BinPackingGame, ItemsGenerator
    from resource_packing_self_play_amd.binpacking.pytorch.NNet import NNetWrapper
    from resource_packing_self_play_amd.utils import dotdict
    rank, w, local = rdist.init_from_env()
    assert w == int(world)
    torch.cuda.set_device(local)
    W, H, N, salt = 10, 10, 8, 29
    args = dotdict(numMCTSSims=16, cpuct=1, alpha=0.75, cuda=True, num_items=N, num_bins=1, epochs=1, batch_size=8, numIters=2, numEps=13,
                   iterStepThreshold=1, binH_min=6, binH=10, numScoresForRank=10, numItersForTrainExamplesHistory=5, maxlenOfQueue=200000,
                   numItems=N, checkpoint=os.path.join(out_dir, "rb_w%s_r%d" % (world, rank)), sample_seed=3000026, use_graph=False, groups=2,
                   tie_salt=salt, rank_buffer="sequential", greedy_tie_break="draw",
                   host_evaluator=host_evaluator(lambda s: "hashed", W * N, lambda s: salt))
    game = BinPackingGame(W, H, N, 1)
    torch.manual_seed(100)
    nnet = NNetWrapper(game, args)
    gen = ItemsGenerator(W, H, N)
    coach = CoachBPP(game, nnet, gen.items_generator(100), W * H, gen, args, saved_rewards_list=[])
    draws = iter([(9, [101 + 7 * k for k in range(13)]), (8, [5 + 3 * k for k in range(13)])])
    coach.drawIteration = lambda: next(draws)
    starts, orig = [], coach.selfPlayIteration

    def recording(i, draws=None, move_rule=None):
        starts.append([float(x) for x in coach.rewards_list])
        return orig(i, draws=draws, move_rule=move_rule)
    coach.selfPlayIteration = recording
    np.random.seed(1234)
    coach.learn()  # the evaluator is the host table, so training does not change the episodes
    out = dict(buffer1=np.array(starts[1]), buffer2=np.array(coach.rewards_list))
    for it in range(2):
        planes, pi, value = coach.trainExamplesHistory[it].dense()
        rec = coach.repair_log[it]
        out.update({"scores%d" % (it + 1): np.array(coach.iteration_scores[it]), "planes%d" % (it + 1): planes.cpu().numpy().astype(np.uint8),
                    "pi%d" % (it + 1): pi.cpu().numpy(), "value%d" % (it + 1): value.cpu().numpy(), "rounds%d" % (it + 1): rec["rounds"],
                    "replayed%d" % (it + 1): np.array(rec["replayed"], np.int64), "bl%d" % (it + 1): rec["bl"],
                    "has_buf%d" % (it + 1): rec["has_buf"]})
    np.savez(os.path.join(out_dir, "rank_buffer_w%s_r%d.npz" % (world, rank)), **out)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
