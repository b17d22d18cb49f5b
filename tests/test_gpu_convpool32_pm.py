"""Position-major 5x5 entry kernel of a 32-channel stage (k_convpool32_pm): conv3x3 32 -> 32 + bias + max_pool2d(3, 2, 1)
with one pixel position of 16 consecutive leaves per tile, so the MFMAs whose input position lies outside the image are not issued.
They only ever added w * 0 and the maximum is exact, so the kernel must reproduce k_convpool32 bit for bit (up to the sign of a zero,
which torch.equal ignores).  RP_CONVPOOL_PM = 1 / 0 forces the new / old kernel; it is read at every call."""
import os

import numpy as np
import pytest

from test_gpu_nnet import GOLDEN, gpu_wrapper

pytestmark = pytest.mark.gpu

SI = 2  # the c3 net's third stage: 32 x 5 x 5 -> 32 x 3 x 3


class _Forced:
    """RP_CONVPOOL_PM for the calls inside the block (None: unset), restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RP_CONVPOOL_PM")
        if self.value is None:
            os.environ.pop("RP_CONVPOOL_PM", None)
        else:
            os.environ["RP_CONVPOOL_PM"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("RP_CONVPOOL_PM", None)
        else:
            os.environ["RP_CONVPOOL_PM"] = self.old


@pytest.fixture(scope="module")
def stage():
    import torch
    from resource_packing_self_play_amd import _lib
    d = np.load(os.path.join(GOLDEN, "nnet_c3_seed0.npz"))
    game, net, args = gpu_wrapper(d)
    eng = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    net.refresh_fused()
    keep = net.nnet.refresh_frags(eng)
    conv = net.nnet.conv_seqs[SI].conv
    assert tuple(conv.weight.shape) == (32, 32, 3, 3)
    yield eng, net, keep
    net.nnet._dense.clear()
    eng.close()


def _run(eng, x, frag, bias, force):
    import torch
    out = torch.empty((x.shape[0], 32, 3, 3), device="cuda").contiguous(memory_format=torch.channels_last)
    with _Forced(force):
        eng.nn_convpool32(x, frag, bias, out)
    torch.cuda.synchronize()
    return out


def _entry(net):
    return net.nnet._dense["entryfrag:%d" % SI], net.nnet.conv_seqs[SI].conv.bias.detach()


@pytest.mark.parametrize("B", (1, 15, 16, 17, 65, 1030))
def test_position_major_entry_reproduces_pixel_major_bits(stage, B):
    """1 030 rows make the old kernel run two tiles per wave; 65 make a short last task."""
    import torch
    import torch.nn.functional as F
    eng, net, _ = stage
    frag, bias = _entry(net)
    torch.manual_seed(5000 + B)
    x = torch.randn(B, 32, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    out_new = _run(eng, x, frag, bias, "1")
    out_old = _run(eng, x, frag, bias, "0")
    assert torch.equal(out_new, out_old)
    with torch.no_grad():
        want = F.max_pool2d(net.nnet.conv_seqs[SI].conv(x), kernel_size=3, stride=2, padding=1)
    err = float((out_new - want).abs().max())
    print("convpool32_pm B=%d: max |delta| %.3e" % (B, err))
    assert err <= 2e-5


def test_real_activations_from_stage_one(stage):
    """x = what stage 1's kernels (k_convpool32 16 -> 32 on 10x10, k_resstage32 on 5x5) make of a seeded batch of 33 rows."""
    import torch
    eng, net, _ = stage
    frag, bias = _entry(net)
    D = net.nnet._dense
    torch.manual_seed(33)
    y = torch.relu(torch.randn(33, 16, 10, 10, device="cuda")).contiguous(memory_format=torch.channels_last)  # many exact zeros
    x1 = torch.empty((33, 32, 5, 5), device="cuda").contiguous(memory_format=torch.channels_last)
    eng.nn_convpool32(y, D["entryfrag:1"], net.nnet.conv_seqs[1].conv.bias.detach(), x1)
    x = torch.empty_like(x1)
    x_relu = torch.empty_like(x1)
    eng.nn_resstage32(x1, D["stagefrag:1"], D["stagebias:1"], x, x_relu)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and bool((x < 0).any())
    for xin in (x, x_relu):  # the stage's output as the evaluator passes it on, and its ReLU: exact zeros next to the border
        assert torch.equal(_run(eng, xin, frag, bias, "1"), _run(eng, xin, frag, bias, "0"))
    assert bool((x_relu == 0).any())


def test_position_major_entry_stays_inside_its_rows(stage):
    """64 rows of NaN behind row B of x, a sentinel behind row B of out: nothing past row B reaches a result or is written."""
    import torch
    eng, net, _ = stage
    frag, bias = _entry(net)
    B = 37  # two whole tasks and a short one
    torch.manual_seed(37)
    xf = torch.randn(B + 64, 32, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    xf[B:] = float("nan")
    outf = torch.full((B + 64, 32, 3, 3), 12345.0, device="cuda").contiguous(memory_format=torch.channels_last)
    with _Forced("1"):
        eng.nn_convpool32(xf[:B], frag, bias, outf[:B])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outf[:B]).all())
    assert bool((outf[B:] == 12345.0).all())
    out_old = _run(eng, xf[:B].clone(memory_format=torch.channels_last), frag, bias, "0")
    assert torch.equal(outf[:B], out_old)


@pytest.mark.parametrize("B", (30000, 64))
def test_dispatch_gives_the_forced_old_result_for_any_pick(stage, B):
    import torch
    eng, net, _ = stage
    frag, bias = _entry(net)
    torch.manual_seed(B)
    x = torch.randn(B, 32, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    assert torch.equal(_run(eng, x, frag, bias, None), _run(eng, x, frag, bias, "0"))


def test_weights_refreshed_in_place_are_followed(stage):
    """New weights packed into the same fragment buffer: the next call computes with them (no fragment kept across calls)."""
    import torch
    import torch.nn.functional as F
    eng, net, _ = stage
    conv = net.nnet.conv_seqs[SI].conv
    bias = conv.bias.detach()
    w1 = conv.weight.detach().contiguous().clone()
    torch.manual_seed(99)
    w2 = (w1 + 0.05 * torch.randn_like(w1)).contiguous()
    frag = torch.empty(9 * 32 * 32, device="cuda")
    x = torch.randn(65, 32, 5, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    outs = []
    for w in (w1, w2):
        eng.nn_pack_conv32(w, frag)
        out = _run(eng, x, frag, bias, "1")
        assert torch.equal(out, _run(eng, x, frag, bias, "0"))
        want = F.max_pool2d(F.conv2d(x, w, bias, padding=1), kernel_size=3, stride=2, padding=1)
        err = float((out - want).abs().max())
        print("convpool32_pm refreshed weights: max |delta| %.3e" % err)
        assert err <= 2e-5
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
