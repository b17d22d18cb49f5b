"""Shared pieces of tests/test_gpu_stage16_pp.py and, run as a program, its child process: RP_STAGE16_TAIL is read once per process, so
the comparison of k_resstage16_pp with k_resstage16<7> (the 100 pixels as seven whole tiles, the arithmetic the new kernel keeps) needs a
process started with RP_STAGE16_TAIL=0.  There RP_STAGE16_PP=1 must give the bits of RP_STAGE16_PP=0, for out and out_relu.
usage: stage16_pp_worker.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# partial first task, one leaf short of a task, exactly one, one into the next, three tasks with a short last one, and one more task than
# the 512 resident workgroups of a 256-CU device hold plus three leaves: a second task per workgroup
BATCHES = (1, 7, 8, 9, 23, 8 * 512 + 3)


class Forced:
    """RP_STAGE16_PP for the calls inside the block (None: unset), restored afterwards; the knob is read at every call."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RP_STAGE16_PP")
        if self.value is None:
            os.environ.pop("RP_STAGE16_PP", None)
        else:
            os.environ["RP_STAGE16_PP"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("RP_STAGE16_PP", None)
        else:
            os.environ["RP_STAGE16_PP"] = self.old


def make_stage(eng, seed=16):
    """A 16-channel stage with random weights and biases (PyTorch's default initialisation): the module for the reference, its four
    convolutions as rp_nn_pack_conv16 fragments and [4][16] biases in execution order."""
    import torch
    from resource_packing_self_play_amd.binpacking.pytorch.BinpackingNNet import _Stage
    torch.manual_seed(seed)
    st = _Stage(16, 16).cuda().float()
    frag4 = torch.empty(4 * 36 * 64, device="cuda")
    bias4 = torch.empty(4 * 16, device="cuda")
    keep = []
    with torch.no_grad():
        for k, conv in enumerate((st.res_block0.conv0, st.res_block0.conv1, st.res_block1.conv0, st.res_block1.conv1)):
            conv.bias.uniform_(-0.5, 0.5)  # the default biases are within 1/12: larger ones so a missing or misplaced bias cannot hide
            wt = conv.weight.detach().contiguous()
            keep.append(wt)
            eng.nn_pack_conv16(wt, frag4[k * 2304:(k + 1) * 2304])
            bias4[k * 16:(k + 1) * 16].copy_(conv.bias.detach())
    torch.cuda.synchronize()
    return st, frag4, bias4, keep


def make_x(B, seed):
    """Random leaves with negative values, some leaves all zeros, some pixels all zeros."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    x = torch.randn(B, 16, 10, 10, device="cuda", generator=g)
    x[B // 2] = 0
    x[::6] = 0
    x[:, :, 3, 9] = 0
    x[B - 1, :, 0, 0] = -1.5
    return x.contiguous(memory_format=torch.channels_last)


def run(eng, frag4, bias4, x, force, relu=True):
    import torch
    out = torch.empty_like(x)
    out_r = torch.empty_like(x) if relu else None
    with Forced(force):
        eng.nn_resstage16(x, frag4, bias4, out, out_r)
    torch.cuda.synchronize()
    return out, out_r


def main():
    import torch
    from resource_packing_self_play_amd import _lib
    assert os.environ.get("RP_STAGE16_TAIL") == "0"
    eng = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    st, frag4, bias4, keep = make_stage(eng)
    for B in BATCHES:
        x = make_x(B, B)
        out_new, relu_new = run(eng, frag4, bias4, x, "1")
        out_old, relu_old = run(eng, frag4, bias4, x, "0")
        same = torch.equal(out_new, out_old) and torch.equal(relu_new, relu_old)
        print("B=%d: max |new - old| %.3e, equal %s" % (B, float((out_new - out_old).abs().max()), same), flush=True)
        assert same, B
        only, _ = run(eng, frag4, bias4, x, "1", relu=False)
        assert torch.equal(only, out_new), B
    eng.close()
    print("stage16_pp_worker: ok")


if __name__ == "__main__":
    main()
