"""Position-paired 16-channel 10x10 stage kernel (k_resstage16_pp): a tile is two pixel positions with the same tap set, of
eight consecutive leaves each, and the MFMAs whose input position lies outside the image are not issued.  They only ever added w * 0, so
the kernel must reproduce k_resstage16<7> (RP_STAGE16_TAIL=0: no tail blocks) bit for bit, up to the sign of a zero, which torch.equal
ignores.  RP_STAGE16_PP = 1 / 0 forces the new / old kernel; it is read at every call.

Against the default k_resstage16<6, true> the four tail pixels 96..99 (row 9, columns 6..9), which that kernel sums in another order,
agree within the stage tolerance.  That kernel's tail pixels differ from the whole-tile kernel's by a rounding in EVERY convolution, and
the next convolution carries the difference one pixel further, so after four convolutions the pixels within three of the tail pixels
(rows 6..9, columns 3..9: 28 pixels, CONE) differ by roundings between any two correct kernels -- they are held to the stage tolerance,
the other 72 pixels to the same bits.  (All 100 pixels are compared bit for bit in the fresh process above.)"""
import ctypes
import os
import subprocess
import sys

import pytest

from stage16_pp_worker import BATCHES, HERE, make_stage, make_x, run

pytestmark = pytest.mark.gpu
TOL = 4e-5  # the stage tolerance of test_gpu_nnet.py
CONE = [r * 10 + c for r in range(6, 10) for c in range(3, 10)]  # pixels that see a tail pixel of an earlier convolution
CLEAR = [p for p in range(100) if p not in CONE]


def _against_tail_kernel(new, old, B):
    """(same bits outside the tail pixels' cone, largest difference inside it, pixels that differ) of channels-last [B, 16, 10, 10] results"""
    import torch
    a, b = new.permute(0, 2, 3, 1).reshape(B, 100, 16), old.permute(0, 2, 3, 1).reshape(B, 100, 16)
    differ = sorted(set(torch.nonzero((a != b).any(dim=2))[:, 1].tolist()))
    return torch.equal(a[:, CLEAR], b[:, CLEAR]), float((a[:, CONE] - b[:, CONE]).abs().max()), differ


@pytest.fixture(scope="module")
def stage():
    import torch
    from resource_packing_self_play_amd import _lib
    eng = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    st, frag4, bias4, keep = make_stage(eng)
    yield eng, st, frag4, bias4, keep
    eng.close()


def test_new_kernel_reproduces_the_whole_tile_kernel_bit_for_bit_in_a_fresh_process():
    env = dict(os.environ, RP_STAGE16_TAIL="0")
    env.pop("RP_STAGE16_PP", None)
    p = subprocess.run([sys.executable, "-X", "faulthandler", os.path.join(HERE, "stage16_pp_worker.py")], env=env, capture_output=True, text=True, timeout=280)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "stage16_pp_worker: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("B", BATCHES)
def test_new_kernel_against_the_default_kernel_and_pytorch(stage, B, relu):
    import torch
    eng, st, frag4, bias4, _ = stage
    x = make_x(B, B)
    out_new, relu_new = run(eng, frag4, bias4, x, "1", relu)
    out_old, relu_old = run(eng, frag4, bias4, x, "0", relu)
    same, cone, differ = _against_tail_kernel(out_new, out_old, B)
    with torch.no_grad():
        want = st.res_block1(st.res_block0(x))
    err = float((out_new - want).abs().max())
    print("resstage16_pp B=%d relu=%s: max |new - old| in the tail pixels' cone %.3e (pixels that differ: %s), max |new - torch| %.3e"
          % (B, relu, cone, differ, err))
    if os.environ.get("RP_STAGE16_TAIL", "1") != "0":
        assert same and cone <= TOL
    else:  # the suite itself runs without tail blocks: all 100 pixels
        assert torch.equal(out_new, out_old)
    assert err <= TOL
    if relu:
        assert torch.equal(relu_new, torch.relu(out_new))
        same_r, cone_r, _ = _against_tail_kernel(relu_new, relu_old, B)
        assert same_r and cone_r <= TOL
    else:
        assert relu_new is None


@pytest.mark.parametrize("limit", (0, 5, 22))
def test_rows_past_the_device_row_limit_stay_untouched(stage, limit):
    """The limit is a device int (the number of waiting leaves while compact rows are on): rows from it on are neither read into a result
    nor written, in whole tasks (limit 0), inside a task (5) and in the last task (B - 1)."""
    import torch
    eng, st, frag4, bias4, _ = stage
    B = 23
    x = make_x(B, 50 + limit)
    full, full_r = run(eng, frag4, bias4, x, "1")
    xn = x.clone(memory_format=torch.channels_last)
    xn[limit:] = float("nan")
    rows = torch.tensor([limit], dtype=torch.int32, device="cuda")
    out = torch.full_like(x, 12345.0)
    out_r = torch.full_like(x, 12345.0)
    eng.L.rp_debug_set_nn_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    eng.L.rp_debug_set_nn_rows.restype = ctypes.c_int
    assert eng.L.rp_debug_set_nn_rows(eng.h, ctypes.c_void_p(rows.data_ptr())) == 0
    try:
        from stage16_pp_worker import Forced
        with Forced("1"):
            eng.nn_resstage16(xn, frag4, bias4, out, out_r)
        torch.cuda.synchronize()
    finally:
        assert eng.L.rp_debug_set_nn_rows(eng.h, None) == 0
    assert torch.equal(out[:limit], full[:limit]) and torch.equal(out_r[:limit], full_r[:limit])
    assert bool((out[limit:] == 12345.0).all()) and bool((out_r[limit:] == 12345.0).all())


def test_dispatch_gives_the_old_result_for_the_flagship_batch(stage):
    """30 000 rows take the new kernel by the cost rule (tests/test_stage16_pp_host.py): outside the tail pixels' cone the old kernel's bits."""
    import torch
    eng, st, frag4, bias4, _ = stage
    B = 30000
    x = make_x(B, 3)
    out_auto, _ = run(eng, frag4, bias4, x, None, relu=False)
    out_new, _ = run(eng, frag4, bias4, x, "1", relu=False)
    assert torch.equal(out_auto, out_new)
    del out_new
    out_old, _ = run(eng, frag4, bias4, x, "0", relu=False)
    same, cone, _ = _against_tail_kernel(out_auto, out_old, B)
    assert same and cone <= TOL
