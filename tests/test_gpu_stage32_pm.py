"""Position-major 32-channel stage kernels (k_resstage32_pm) for 3x3 and 5x5 images: a tile is one pixel position of 16
consecutive leaves, and the MFMAs whose input position lies outside the image are not issued.  They only ever added w * 0, so the
new kernels must reproduce k_resstage32 bit for bit (up to the sign of a zero, which torch.equal ignores).  RP_STAGE32_PM = 1 / 0
forces the new / old kernel; it is read at every call."""
import os

import numpy as np
import pytest

from stage_shapes import STAGE32_PM_BATCHES as BATCHES
from test_gpu_nnet import GOLDEN, gpu_wrapper

pytestmark = pytest.mark.gpu

CASES = [(S, si, B) for S in (3, 5) for si in (1, 2) for B in BATCHES[S]]


class _Forced:
    """RP_STAGE32_PM for the calls inside the block (None: unset), restored afterwards."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RP_STAGE32_PM")
        if self.value is None:
            os.environ.pop("RP_STAGE32_PM", None)
        else:
            os.environ["RP_STAGE32_PM"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("RP_STAGE32_PM", None)
        else:
            os.environ["RP_STAGE32_PM"] = self.old


@pytest.fixture(scope="module")
def stage():
    import torch
    from resource_packing_self_play_amd import _lib
    d = np.load(os.path.join(GOLDEN, "nnet_c3_seed0.npz"))
    game, net, args = gpu_wrapper(d)
    eng = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    net.refresh_fused()
    keep = net.nnet.refresh_frags(eng)
    yield eng, net, keep
    net.nnet._dense.clear()
    eng.close()


def _run(eng, net, si, x, force, relu=True):
    import torch
    frag4, bias4 = net.nnet._dense["stagefrag:%d" % si], net.nnet._dense["stagebias:%d" % si]
    out = torch.empty_like(x)
    out_r = torch.empty_like(x) if relu else None
    with _Forced(force):
        eng.nn_resstage32(x, frag4, bias4, out, out_r)
    torch.cuda.synchronize()
    return out, out_r


@pytest.mark.parametrize("S,si,B", CASES)
def test_position_major_kernel_reproduces_pixel_major_bits(stage, S, si, B):
    import torch
    eng, net, _ = stage
    torch.manual_seed(1000 * S + 100 * si + B)
    x = torch.randn(B, 32, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
    out_new, relu_new = _run(eng, net, si, x, "1")
    out_old, relu_old = _run(eng, net, si, x, "0")
    assert torch.equal(out_new, out_old) and torch.equal(relu_new, relu_old)
    assert torch.equal(relu_new, torch.relu(out_new))
    out_only, _ = _run(eng, net, si, x, "1", relu=False)
    assert torch.equal(out_only, out_new)
    st = net.nnet.conv_seqs[si]
    with torch.no_grad():
        want = st.res_block1(st.res_block0(x))
    err = float((out_new - want).abs().max())
    print("resstage32_pm stage %d B=%d %dx%d: max |delta| %.3e" % (si, B, S, S, err))
    assert err <= 4e-5


@pytest.mark.parametrize("S", (3, 5))
def test_position_major_kernel_stays_inside_its_rows(stage, S):
    """64 rows of NaN behind row B of x, a sentinel behind row B of both outputs: nothing past row B reaches a result or is written."""
    import torch
    eng, net, _ = stage
    B, si = 37, 1  # two whole tasks and a short one
    torch.manual_seed(7 + S)
    xf = torch.randn(B + 64, 32, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
    xf[B:] = float("nan")
    frag4, bias4 = net.nnet._dense["stagefrag:%d" % si], net.nnet._dense["stagebias:%d" % si]
    outf = torch.full_like(xf, 12345.0)
    relf = torch.full_like(xf, 12345.0)
    with _Forced("1"):
        eng.nn_resstage32(xf[:B], frag4, bias4, outf[:B], relf[:B])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outf[:B]).all()) and bool(torch.isfinite(relf[:B]).all())
    assert bool((outf[B:] == 12345.0).all()) and bool((relf[B:] == 12345.0).all())
    out_old, relu_old = _run(eng, net, si, xf[:B].clone(memory_format=torch.channels_last), "0")
    assert torch.equal(outf[:B], out_old) and torch.equal(relf[:B], relu_old)


@pytest.mark.parametrize("B", (30000, 64))
def test_dispatch_gives_the_forced_old_result_for_any_pick(stage, B):
    import torch
    eng, net, _ = stage
    torch.manual_seed(B)
    x = torch.randn(B, 32, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last)
    out_auto, relu_auto = _run(eng, net, 2, x, None)
    out_old, relu_old = _run(eng, net, 2, x, "0")
    assert torch.equal(out_auto, out_old) and torch.equal(relu_auto, relu_old)
