"""Row limit, write bounds and leaf isolation of every CNN stage kernel instantiation (the rows contract).

BatchedSelfPlay runs with compact rows: every stage kernel reads the number of waiting leaves from a device int and lowers its B to it,
while grid, LDS and leaves per wave or workgroup were planned by the host for the host's B.  What happens at the last, partly filled
group of leaves therefore rests on each kernel's own code.  Per launch shape (stage_shapes.row_limit_cases: every shape of the stage
tests under both values of its entry point's per-call knob; test_stage_plans_host.py checks that they reach all 53 instantiations), with
out_relu given and without:

  1. guards      x, out and out_relu are views [2 : 2 + B] of buffers with two guard rows on each side; the outputs are pre-filled
                 with a sentinel bit pattern, the guard rows of x are NaN.  Afterwards every guard row holds its bits and x is unchanged.
  2. row limit   for L in {0, 1, g - 1, g, g + 1, 4 g, B - 1, B, B + 7} (g = the plan's leaves per wave or workgroup) the device int is
                 L and the rows of x from min(L, B) on are NaN: rows below the limit equal the unlimited run of the same kernel bit
                 for bit, rows from it on and the guards keep the sentinel.
  3. isolation   one whole leaf j in {0, g - 1, g, B // 2, B - 1} is NaN: every other row equals the clean run bit for bit.

The clean run is also held to the float64 CPU evaluation of the same module on rows [0 : 32] and [B - 8 : B], at the stage tolerances
of test_gpu_nnet.py (4e-5 residual stages, 2e-5 conv + pool), which removes MIOpen's own float32 error from the reference.

Measured on an MI355X, worst element over all cases of a family, |hip - f64| beside |PyTorch-CPU float32 - f64| on the same rows:
    k_resstage16     4.95e-07  4.41e-07      k_resstage32     4.76e-07  5.73e-07      k_convpool32     1.51e-06  1.59e-06
    k_resstage16_wg  4.78e-07  4.51e-07      k_resstage32_wg  5.92e-07  5.37e-07      k_convpool32_wg  1.55e-06  1.51e-06
    k_resstage16_pp  4.18e-07  4.91e-07      k_resstage32_pm  5.69e-07  5.04e-07      k_convpool32_pm  1.34e-06  1.48e-06
-- the kernels are as close to the float64 result as PyTorch's float32 CPU convolutions, a factor of 13 to 80 inside the tolerances
(the tolerances are not tightened here: the ratio between an MFMA k-chain and the CPU's blocked summation is not known yet).

rp_nn_resblock16 has no row limit: checks 1 and 3 at the shapes of test_fused_resblock16_kernel_matches_pytorch_block."""
import copy
import ctypes
import os

import numpy as np
import pytest

import stage_shapes
from stage16_pp_worker import Forced as _ForcedStage16
from test_gpu_convpool32_pm import _Forced as _ForcedConvpool
from test_gpu_nnet import GOLDEN, gpu_wrapper
from test_gpu_stage32_pm import _Forced as _ForcedStage32

pytestmark = pytest.mark.gpu

G = 2  # guard rows on each side
SENTINEL = 12345.0
FAMILIES = ["none", "k_resstage16", "k_resstage16_wg", "k_resstage32", "k_resstage32_wg", "k_resstage32_pm", "k_convpool32", "k_convpool32_wg",
            "k_convpool32_pm", "k_resstage16_pp"]  # the planner's family numbers
TOL = {stage_shapes.ENTRY_RESSTAGE16: 4e-5, stage_shapes.ENTRY_CONVPOOL32: 2e-5, stage_shapes.ENTRY_RESSTAGE32: 4e-5}
FORCED = (_ForcedStage16, _ForcedConvpool, _ForcedStage32)  # by entry
# both 32-channel stages for rp_nn_resstage32 (si 1 and 2 of the c3 net), the 16-channel stage (si 0) for rp_nn_resstage16
CASES = [c + (si,) for c in stage_shapes.row_limit_cases()
         for si in ((1, 2) if c[0] == stage_shapes.ENTRY_RESSTAGE32 else (0,) if c[0] == stage_shapes.ENTRY_RESSTAGE16 else (-1,))]
WORST = {}  # family -> [worst |hip - f64|, worst |cpu32 - f64|]


def _case_id(c):
    entry, cin, B, H, W, knob, si = c
    return "%s-cin%d-B%d-%dx%d-knob%d%s" % (("resstage16", "convpool32", "resstage32")[entry], cin, B, H, W, knob, "-si%d" % si if si > 0 else "")


@pytest.fixture(scope="module")
def kit():
    import torch
    from resource_packing_self_play_amd import _lib
    d = np.load(os.path.join(GOLDEN, "nnet_c3_seed0.npz"))
    game, net, args = gpu_wrapper(d)
    eng = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    net.refresh_fused()
    keep = net.nnet.refresh_frags(eng)
    torch.manual_seed(6)
    convs = {}
    for cin in (16, 32):  # the entry convolutions, as in test_fused_convpool32_kernel_matches_pytorch_conv_and_pool
        conv = torch.nn.Conv2d(cin, 32, 3, padding=1).cuda()
        frag = torch.empty(9 * cin * 32, device="cuda")
        wt = conv.weight.detach().contiguous()
        keep.append(wt)
        eng.nn_pack_conv32(wt, frag)
        convs[cin] = (conv, frag)
    torch.cuda.synchronize()
    L = eng.L
    i32, i64, out_t = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.rp_debug_stage_plan.argtypes = [i32, i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_convpool_plan.argtypes = [i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_stage16_plan.argtypes = [i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_set_nn_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.rp_debug_set_nn_rows.restype = ctypes.c_int
    prop = torch.cuda.get_device_properties(0)
    n_cu = int(prop.multi_processor_count)
    lds = max(160 * 1024 if "gfx950" in getattr(prop, "gcnArchName", "") else 64 * 1024, int(getattr(prop, "shared_memory_per_multiprocessor", 0)))
    env_int = lambda name, unset: int(os.environ.get(name, unset))  # the per-process knobs, as the launchers read them
    wgs = (env_int("RP_STAGE16_WGS", 2), env_int("RP_CONVPOOL_WGS", 2), env_int("RP_STAGE32_WGS", 2))
    tail = (env_int("RP_STAGE16_TAIL", 1), env_int("RP_CONVPOOL_TAIL", 1), 0)

    def plan(entry, cin, B, H, W, knob):
        """(family name, leaves per wave or workgroup) of the launch"""
        out = (ctypes.c_int64 * 10)()
        if entry == stage_shapes.ENTRY_RESSTAGE16:
            rc = L.rp_debug_stage16_plan(B, H, W, n_cu, lds, wgs[0], tail[0], knob, out)
        elif entry == stage_shapes.ENTRY_CONVPOOL32:
            rc = L.rp_debug_convpool_plan(cin, B, H, W, n_cu, lds, wgs[1], tail[1], knob, out)
        else:
            rc = L.rp_debug_stage_plan(entry, cin, B, H, W, n_cu, lds, wgs[2], tail[2], knob, out)
        assert rc == 0 and out[5] >= 1
        return FAMILIES[out[0]], int(out[5])

    refs = {}

    def module(entry, cin, si):
        """(GPU module, its float64 and float32 copies on the CPU) of the operation, x -> result"""
        import torch.nn.functional as F
        key = (entry, cin, si)
        if key not in refs:
            if entry == stage_shapes.ENTRY_CONVPOOL32:
                mods = [convs[cin][0], copy.deepcopy(convs[cin][0]).double().cpu(), copy.deepcopy(convs[cin][0]).float().cpu()]
                refs[key] = [lambda x, m=m: F.max_pool2d(m(x), kernel_size=3, stride=2, padding=1) for m in mods]
            else:
                st = net.nnet.conv_seqs[si]
                mods = [st, copy.deepcopy(st).double().cpu(), copy.deepcopy(st).float().cpu()]
                refs[key] = [lambda x, m=m: m.res_block1(m.res_block0(x)) for m in mods]
        return refs[key]

    def launch(case, x, out, out_relu):
        entry, cin, B, H, W, knob, si = case
        D = net.nnet._dense
        with FORCED[entry](str(knob)):
            if entry == stage_shapes.ENTRY_RESSTAGE16:
                eng.nn_resstage16(x, D["stagefrag:0"], D["stagebias:0"], out, out_relu)
            elif entry == stage_shapes.ENTRY_CONVPOOL32:
                eng.nn_convpool32(x, convs[cin][1], convs[cin][0].bias.detach(), out)
            else:
                eng.nn_resstage32(x, D["stagefrag:%d" % si], D["stagebias:%d" % si], out, out_relu)
        torch.cuda.synchronize()

    yield dict(eng=eng, net=net, plan=plan, module=module, launch=launch, keep=keep)
    if WORST:
        print("\nworst |hip - f64| / |cpu32 - f64| per family:")
        for fam in sorted(WORST):
            print("    %-16s %.3e  %.3e" % (fam, WORST[fam][0], WORST[fam][1]))
    net.nnet._dense.clear()
    eng.close()


def _guarded(shape, fill):
    """a channels-last [B + 2 G, C, H, W] buffer of `fill` and its rows [G : G + B]"""
    import torch
    B, C, H, W = shape
    buf = torch.full((B + 2 * G, C, H, W), fill, device="cuda").contiguous(memory_format=torch.channels_last)
    return buf, buf[G:G + B]


def _bits(t):
    import torch
    return t.view(torch.int32)


SENTINEL_BITS = int(np.float32(SENTINEL).view(np.int32))


def _holds_sentinel(t):
    return bool((_bits(t) == SENTINEL_BITS).all())


def _same_bits(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


class _RowLimit:
    """the device row limit of the engine's stage launches for the block, none afterwards"""

    def __init__(self, eng, limit):
        import torch
        self.eng = eng
        self.rows = torch.tensor([limit], dtype=torch.int32, device="cuda")

    def __enter__(self):
        assert self.eng.L.rp_debug_set_nn_rows(self.eng.h, ctypes.c_void_p(self.rows.data_ptr())) == 0

    def __exit__(self, *exc):
        import torch
        try:
            torch.cuda.synchronize()
        finally:
            assert self.eng.L.rp_debug_set_nn_rows(self.eng.h, None) == 0


def _three_checks(run, x_shape, out_shape, g, B, seed, limits=True, has_relu=True):
    """Checks 1 to 3 of the module docstring for run(x, out, out_relu); returns (clean x, clean out) for the float64 comparison."""
    import torch
    nan = float("nan")
    torch.manual_seed(seed)
    xbuf, x = _guarded(x_shape, nan)
    x.copy_(torch.randn(x_shape, device="cuda"))
    clean = xbuf.clone(memory_format=torch.preserve_format)
    first = None
    for relu in ((True, False) if has_relu else (False,)):
        obuf, out = _guarded(out_shape, SENTINEL)
        rbuf, out_r = _guarded(out_shape, SENTINEL) if relu else (None, None)
        outs = [(obuf, out)] + ([(rbuf, out_r)] if relu else [])
        # 1. guards
        run(x, out, out_r)
        assert _same_bits(xbuf, clean), "x was written"
        for buf, _ in outs:
            assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + B:]), "a guard row of an output was written"
        assert bool(torch.isfinite(out).all()) and not bool((_bits(out) == SENTINEL_BITS).any()), "a row was not written"
        full = [v.clone(memory_format=torch.preserve_format) for _, v in outs]
        if relu:
            assert torch.equal(full[1], torch.relu(full[0]))
        if first is None:
            first = full[0]
        else:
            assert torch.equal(full[0], first), "out depends on whether out_relu is given"
        # 2. row limit
        if limits:
            for L in sorted({v for v in (0, 1, g - 1, g, g + 1, 4 * g, B - 1, B, B + 7) if v >= 0}):
                m = min(L, B)
                xn = clean.clone(memory_format=torch.preserve_format)
                xn[G + m:] = nan
                for buf, _ in outs:
                    buf.fill_(SENTINEL)
                with _RowLimit(run.eng, L):
                    run(xn[G:G + B], out, out_r)
                for (buf, v), want in zip(outs, full):
                    assert torch.equal(v[:m], want[:m]), "limit %d: a row below the limit differs from the unlimited run" % L
                    assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + m:]), "limit %d: a row from the limit on was written" % L
        # 3. leaf isolation
        for j in sorted({v for v in (0, g - 1, g, B // 2, B - 1) if 0 <= v < B}):
            xp = clean.clone(memory_format=torch.preserve_format)
            xp[G + j] = nan
            for buf, _ in outs:
                buf.fill_(SENTINEL)
            run(xp[G:G + B], out, out_r)
            for (buf, v), want in zip(outs, full):
                assert torch.equal(v[:j], want[:j]) and torch.equal(v[j + 1:], want[j + 1:]), "leaf %d reached another leaf's result" % j
                assert _holds_sentinel(buf[:G]) and _holds_sentinel(buf[G + B:])
    return x, first


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_row_limit_write_bounds_and_leaf_isolation(kit, case):
    import torch
    entry, cin, B, H, W, knob, si = case
    fam, g = kit["plan"](entry, cin, B, H, W, knob)
    pooled = entry == stage_shapes.ENTRY_CONVPOOL32
    out_shape = (B, 32, (H + 1) // 2, (W + 1) // 2) if pooled else (B, cin, H, W)

    def run(x, out, out_relu):
        kit["launch"](case, x, out, out_relu)
    run.eng = kit["eng"]
    x, out = _three_checks(run, (B, cin, H, W), out_shape, g, B, seed=7000 + CASES.index(case), has_relu=not pooled)
    # the clean run against the float64 evaluation of the same module
    idx = sorted(set(range(min(32, B))) | set(range(max(0, B - 8), B)))
    assert len(idx) <= 40
    _, f64, f32 = kit["module"](entry, cin, si)
    xs = x[idx].cpu()
    with torch.no_grad():
        want = f64(xs.double())
        cpu32 = f32(xs)
    err = float((out[idx].cpu().double() - want).abs().max())
    err_cpu = float((cpu32.double() - want).abs().max())
    print("%s %s g=%d: max |hip - f64| %.3e, max |cpu32 - f64| %.3e" % (_case_id(case), fam, g, err, err_cpu))
    w = WORST.setdefault(fam, [0.0, 0.0])
    w[0], w[1] = max(w[0], err), max(w[1], err_cpu)
    assert err <= TOL[entry]


@pytest.mark.parametrize("B,H,W", [(5, 10, 10), (1030, 10, 10), (64, 7, 9), (33, 3, 3), (17, 13, 12)])
def test_resblock16_write_bounds_and_leaf_isolation(kit, B, H, W):
    """rp_nn_resblock16: one leaf per wave, four per workgroup, no row limit."""
    import torch
    eng, blk = kit["eng"], kit["net"].nnet.conv_seqs[0].res_block1
    f0 = torch.empty(36 * 64, device="cuda"); f1 = torch.empty(36 * 64, device="cuda")
    w0, w1 = blk.conv0.weight.detach().contiguous(), blk.conv1.weight.detach().contiguous()
    eng.nn_pack_conv16(w0, f0); eng.nn_pack_conv16(w1, f1)

    def run(x, out, out_relu):
        eng.nn_resblock16(x, f0, blk.conv0.bias.detach(), f1, blk.conv1.bias.detach(), out, out_relu)
        torch.cuda.synchronize()
    run.eng = eng
    _three_checks(run, (B, 16, H, W), (B, 16, H, W), 4, B, seed=300 + B + H, limits=False)
