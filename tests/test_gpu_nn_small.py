"""The small kernels behind the stage kernels, each on its own: rp_nn_bias_relu, rp_nn_bias_residual and the three rp_nn_bias_pool kernels
(NCHW, scalar channels-last for C % 4 != 0, four channels per thread) against an exactly rounded reference, rp_nn_value_head against the
float64 dot product, and the argument checks of their _lib.Engine wrappers.

Element-wise kernels: every output element is one float32 add (one more for the skip) and comparisons, so the reference is exact --
float64 x + b rounded once to float32 (innocuous: 53 >= 2 * 24 + 2 bits), + res the same way, then max_pool2d(3, 2, 1) / relu on the CPU --
and the comparison is torch.equal (the sign of a zero is ignored, as elsewhere in this suite).  Inputs: randn; round(4 randn) / 4 (ties);
all-negative data with a negative bias (a maximum seeded with 0, or a dropped border test, shows); mixed magnitudes 10^-20 .. 10^20 with a
bias of 1e4, where distinct inputs round to the same sum (the four-channel pool kernel adds the bias after the maximum:
max(fl(x_i + b)) == fl(max(x_i) + b)).  No input, and no sum, is a NaN, an infinity or a denormal (asserted).  Outputs are views into
sentinel buffers with at least one guard row on each side.

Value head: out = tanh(z . w + bias) with one wave per row, a lane summing K / 4 / 64 (rounded up) float4 products, six shuffle adds, the
bias add: |out - tanh(float64 dot + bias)| <= gamma_n (sum |z_i w_i| + |bias|) + T_ULPS * 2^-24 with n = 4 ceil(K / 256) + 7,
gamma_n = n u / (1 - n u), u = 2^-24 (tanh is 1-Lipschitz).  T_ULPS, the tanhf allowance in ulps of a result below 1: the ROCm
installation ships no document that states a bound for tanhf, so it is the worst error of torch.tanh on float32 CPU tensors against
float64 tanh over 10^6 evenly spaced points of [-10, 10], 0.535 ulp (at x = -1.2494), plus 2 ulps for a different libm: 2.54.
Measured on an MI355X: the worst |out - ref| is 0.135 of the bound (K = 4; 0.008 at K = 4 096 -- the bound is a worst case over the
roundings), 1.5 to 6.7 x 2^-24 on the relu(randn) rows, and within the tanhf allowance on the rows of zeros."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
SHAPES = [(1, 4, 1, 1), (3, 16, 1, 1), (4, 32, 1, 1), (5, 16, 3, 3), (7, 32, 5, 5), (2, 6, 2, 3), (1, 1, 1, 4), (33, 32, 2, 2), (9, 16, 1, 7), (9, 16, 7, 1),
          (6, 32, 2, 9), (5, 16, 4, 4), (5, 16, 6, 10), (257, 16, 7, 9), (3, 32, 13, 13), (2, 16, 13, 25), (4, 3, 5, 4), (4, 6, 9, 9)]
QUAD_SHAPES = [s for s in SHAPES if (s[0] * s[1] * s[2] * s[3]) % 4 == 0]  # bias_relu / bias_residual move 16 bytes per thread
KINDS = ("randn", "ties", "negative", "magnitudes")
T_ULPS = 2.54  # tanhf allowance (module docstring)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    import torch
    from resource_packing_self_play_amd import _lib
    e = _lib.Engine(20, 20, 32, 1, 1, stream=torch.cuda.current_stream().cuda_stream)
    yield e
    e.close()


def _normal(t):
    import torch
    return bool(torch.isfinite(t).all()) and bool(((t.abs() >= torch.finfo(torch.float32).tiny) | (t == 0)).all())


def _inputs(kind, shape, seed):
    """(x, bias, res) on the CPU, float32, under their own seed"""
    import torch
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    rn = lambda s: torch.randn(s, generator=g)
    if kind == "randn":
        x, b, r = rn(shape), rn((C,)), rn(shape)
    elif kind == "ties":
        x, b, r = torch.round(4 * rn(shape)) / 4, torch.round(4 * rn((C,))) / 4, torch.round(4 * rn(shape)) / 4
    elif kind == "negative":
        x, b, r = -torch.rand(shape, generator=g) - 0.5, -torch.rand((C,), generator=g) - 0.5, -torch.rand(shape, generator=g) - 0.5
    else:
        mag = lambda s: (rn(s).double() * 10.0 ** torch.randint(-20, 21, s, generator=g).double()).float()
        x, b, r = mag(shape), torch.full((C,), 1e4), mag(shape)
    assert _normal(x) and _normal(b) and _normal(r)
    return x, b, r


def _add_bias(x, b):
    """fl(x + b[c]): the float64 sum rounded once"""
    s = (x.double() + b.double().view(1, -1, 1, 1)).float()
    assert _normal(s)
    return s


def _place(t, cl):
    """t on the device in NCHW or channels-last order"""
    import torch
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if cl else t.contiguous()


def _guarded(shape, cl):
    """A flat sentinel buffer and the [B, C, H, W] view (NCHW or channels-last) of its middle, 16-byte aligned, with at least one row of
    guard elements on each side; returns (view, guards)."""
    import torch
    B, C, H, W = shape
    row = C * H * W
    front = (row + 3) // 4 * 4
    flat = torch.full((front + B * row + row,), SENTINEL, device="cuda")
    body = flat[front:front + B * row]
    view = body.view(B, H, W, C).permute(0, 3, 1, 2) if cl else body.view(B, C, H, W)
    return view, (flat[:front], flat[front + B * row:])


def _untouched(guards):
    import torch
    want = int(np.float32(SENTINEL).view(np.int32))
    return all(bool((g.view(torch.int32) == want).all()) for g in guards)


def _layouts(shape):
    """channels-last differs from NCHW only with more than one channel and more than one pixel"""
    return (False, True) if shape[1] > 1 and shape[2] * shape[3] > 1 else (False,)


@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_relu_is_exactly_rounded(eng, shape):
    import torch
    for k, kind in enumerate(KINDS):
        x, b, _ = _inputs(kind, shape, 1000 * k + sum(shape))
        want = torch.relu(_add_bias(x, b))
        for cl in _layouts(shape):
            view, guards = _guarded(shape, cl)
            view.copy_(x.cuda())
            got = eng.nn_bias_relu(view, b.cuda())
            torch.cuda.synchronize()
            assert got is view and torch.equal(view.cpu(), want), (kind, cl)
            assert _untouched(guards), (kind, cl)
        if kind == "negative":
            assert not bool(want.any())


@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_residual_is_exactly_rounded(eng, shape):
    import torch
    for k, kind in enumerate(KINDS):
        x, b, r = _inputs(kind, shape, 2000 * k + sum(shape))
        want = (_add_bias(x, b).double() + r.double()).float()
        assert _normal(want)
        for cl in _layouts(shape):
            xd, rd, bd = _place(x, cl), _place(r, cl), b.cuda()
            for relu in (True, False):
                out, guards = _guarded(shape, cl)
                out_r, guards_r = _guarded(shape, cl) if relu else (None, ())
                eng.nn_bias_residual(xd, bd, rd, out, out_r)
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), want), (kind, cl, relu)
                assert _untouched(guards) and _untouched(guards_r), (kind, cl, relu)
                if relu:
                    assert torch.equal(out_r.cpu(), torch.relu(want)), (kind, cl)
            assert torch.equal(xd.cpu(), x) and torch.equal(rd.cpu(), r)  # the inputs stay


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_pool_is_exactly_rounded_in_all_three_kernels(eng, shape):
    """NCHW: k_nn_bias_pool; channels-last with C % 4 != 0: k_nn_bias_pool_nhwc; with C % 4 == 0: k_nn_bias_pool_nhwc4."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = shape
    pooled = (B, C, (H + 1) // 2, (W + 1) // 2)
    for k, kind in enumerate(KINDS):
        x, b, _ = _inputs(kind, shape, 3000 * k + sum(shape))
        want = F.max_pool2d(_add_bias(x, b), kernel_size=3, stride=2, padding=1)
        assert tuple(want.shape) == pooled
        if kind == "negative":
            assert bool((want < 0).all())
        if kind == "magnitudes":  # the claim behind the bias-after-maximum kernel, on the reference's own numbers
            assert torch.equal(want, _add_bias(F.max_pool2d(x, kernel_size=3, stride=2, padding=1), b))
        for cl in _layouts(shape):
            xd, bd = _place(x, cl), b.cuda()
            for relu in (True, False):
                out, guards = _guarded(pooled, cl)
                out_r, guards_r = _guarded(pooled, cl) if relu else (None, ())
                eng.nn_bias_pool(xd, bd, out, out_r)
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), want), (kind, cl, relu)
                assert _untouched(guards) and _untouched(guards_r), (kind, cl, relu)
                if relu:
                    assert torch.equal(out_r.cpu(), torch.relu(want)), (kind, cl)
                    if kind == "negative":
                        assert not bool(out_r.any())
            assert torch.equal(xd.cpu(), x)


def test_element_counts_that_are_no_multiple_of_four_are_refused_and_empty_batches_do_nothing(eng):
    import torch
    from resource_packing_self_play_amd._lib import ERR_ARG, EngineError
    for shape in ((1, 1, 1, 3), (3, 6, 3, 3), (5, 3, 5, 5)):
        x = torch.full(shape, SENTINEL, device="cuda")
        b = torch.zeros(shape[1], device="cuda")
        out = torch.full(shape, SENTINEL, device="cuda")
        with pytest.raises(EngineError) as e:
            eng.nn_bias_relu(x, b)
        assert e.value.code == ERR_ARG
        with pytest.raises(EngineError) as e:
            eng.nn_bias_residual(x, b, x.clone(), out, None)
        assert e.value.code == ERR_ARG
        torch.cuda.synchronize()
        assert bool((x == SENTINEL).all()) and bool((out == SENTINEL).all())  # refused before any launch
    for cl in (False, True):
        fmt = torch.channels_last if cl else torch.contiguous_format
        x = torch.empty((0, 16, 5, 5), device="cuda").contiguous(memory_format=fmt)
        b = torch.zeros(16, device="cuda")
        assert eng.nn_bias_relu(x, b) is x
        eng.nn_bias_residual(x, b, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x))
        p = torch.empty((0, 16, 3, 3), device="cuda").contiguous(memory_format=fmt)
        eng.nn_bias_pool(x, b, p, torch.empty_like(p))
    eng.nn_value_head(torch.empty((0, 8), device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(1, device="cuda"), torch.empty(0, device="cuda"))
    torch.cuda.synchronize()


def test_wrappers_refuse_tensors_of_another_type_place_shape_or_memory_order(eng):
    """A tensor in another memory order than x would be indexed as if it had x's: ValueError before any launch."""
    import torch
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x = torch.randn(4, 8, 5, 5, device="cuda")
    b = torch.randn(8, device="cuda")
    out, out_r = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
    p, p_r = torch.full((4, 8, 3, 3), SENTINEL, device="cuda"), torch.full((4, 8, 3, 3), SENTINEL, device="cuda")
    bad_calls = [
        lambda: eng.nn_bias_relu(x.double(), b), lambda: eng.nn_bias_relu(x, b.double()), lambda: eng.nn_bias_relu(x.cpu(), b),
        lambda: eng.nn_bias_relu(x, b.cpu()), lambda: eng.nn_bias_relu(x, b[:4]), lambda: eng.nn_bias_relu(x, torch.randn(16, device="cuda")[::2]),
        lambda: eng.nn_bias_relu(x[:, :, ::2], b), lambda: eng.nn_bias_relu(x.permute(0, 1, 3, 2), b),
        lambda: eng.nn_bias_residual(x, b, cl(x), out, out_r), lambda: eng.nn_bias_residual(x, b, x, cl(out), out_r),
        lambda: eng.nn_bias_residual(x, b, x, out, cl(out_r)), lambda: eng.nn_bias_residual(cl(x), b, x, out, out_r),
        lambda: eng.nn_bias_residual(x, b, x[:3], out, out_r), lambda: eng.nn_bias_residual(x, b, x, out[:, :4], None),
        lambda: eng.nn_bias_residual(x, b, x.double(), out, None), lambda: eng.nn_bias_residual(x, b, x, out.cpu(), None),
        lambda: eng.nn_bias_pool(x, b, cl(p), p_r), lambda: eng.nn_bias_pool(x, b, p, cl(p_r)), lambda: eng.nn_bias_pool(cl(x), b, p, None),
        lambda: eng.nn_bias_pool(x, b, out, None), lambda: eng.nn_bias_pool(x, b, p[:, :, :2], None), lambda: eng.nn_bias_pool(x, b, p, p_r.double()),
        lambda: eng.nn_bias_pool(x, b[:4], p, None), lambda: eng.nn_bias_pool(x.view(4, 8, 25), b, p, None),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for t in (out, out_r, p, p_r):
        assert bool((t == SENTINEL).all())
    # where the two orders coincide (one channel, or a 1x1 image), either is accepted
    for shape in ((4, 1, 2, 6), (12, 8, 1, 1)):
        y = torch.randn(shape, device="cuda")
        bb = torch.randn(shape[1], device="cuda")
        want = (y + bb.view(1, -1, 1, 1)) + y
        for a in (y, cl(y)):
            for o in (torch.empty_like(y), cl(torch.empty_like(y))):
                eng.nn_bias_residual(a, bb, cl(y), o, None)
                assert torch.equal(o, want)
    y = cl(torch.randn(4, 8, 2, 2, device="cuda"))  # a 1x1 pooled image behind a channels-last x
    for o in (torch.empty(4, 8, 1, 1, device="cuda"), cl(torch.empty(4, 8, 1, 1, device="cuda"))):
        eng.nn_bias_pool(y, b, o, None)
        assert torch.equal(o, torch.nn.functional.max_pool2d(y + b.view(1, -1, 1, 1), 3, 2, 1))


@pytest.mark.parametrize("K", (4, 8, 252, 256, 260, 512, 1028, 4096))
def test_value_head_within_the_bound_of_its_own_arithmetic(eng, K):
    """Rows of relu(randn) (what hidden_fc produces) with one row of zeros, and the same rows scaled so that the pre-activations
    reach +-15 (saturation); w as [1, K] and as [K]; out with guard elements on both sides.  Bound and T_ULPS: module docstring."""
    import torch
    n = 4 * math.ceil(K / 256) + 7
    gamma = n * U / (1 - n * U)
    worst, worst_plain = 0.0, 0.0  # largest |out - ref| / bound, largest |out - ref| of the unscaled rows in units of 2^-24
    for B in (1, 2, 3, 4, 5, 63, 1027):
        g = torch.Generator().manual_seed(100 * K + B)
        z = torch.relu(torch.randn((B, K), generator=g))
        w = torch.randn((K,), generator=g) / math.sqrt(K)
        bias = torch.randn((1,), generator=g) * 0.5
        zero = B // 2 if B > 1 else None  # the row of zeros
        if zero is not None:
            z[zero] = 0
        dot = z.double() @ w.double()
        target = torch.linspace(0.01, 15.0, B, dtype=torch.float64)
        zs = (z.double() * (target / dot.abs().clamp_min(1e-30)).view(-1, 1)).float()  # |pre-activation - bias| = target, the dot product's sign
        if zero is not None:
            zs[zero] = 0
        for rows in (z, zs):
            assert _normal(rows)
            absdot = rows.double().abs() @ w.double().abs()
            pre = rows.double() @ w.double() + bias.double()
            ref = torch.tanh(pre)
            if rows is zs and B >= 63:
                assert float(pre.min()) < -10 and float(pre.max()) > 10
            bound = gamma * (absdot + bias.double().abs()) + T_ULPS * U
            zd, bd = rows.cuda(), bias.cuda()
            for wd in (w.cuda().view(1, K), w.cuda()):
                buf = torch.full((B + 8,), SENTINEL, device="cuda")
                out = buf[4:4 + B]
                eng.nn_value_head(zd, wd, bd, out)
                torch.cuda.synchronize()
                got = out.cpu().double()
                assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + B:] == SENTINEL).all())
                assert bool((got.abs() <= 1).all())
                err = (got - ref).abs()
                over = err - bound
                worst = max(worst, float((err / bound).max()))
                if rows is z:
                    worst_plain = max(worst_plain, float((err / U).max()))
                assert float(over.max()) <= 0, "K %d B %d row %d: |out - ref| %.3e over the bound %.3e" % (
                    K, B, int(over.argmax()), float(err[over.argmax()]), float(bound[over.argmax()]))
                if zero is not None:  # acc = 0 and 0 + bias are exact: tanhf's error alone
                    assert abs(float(got[zero]) - math.tanh(float(bias))) <= T_ULPS * U
            out2 = torch.empty((B, 1), device="cuda")
            eng.nn_value_head(zd, w.cuda().view(1, K), bd, out2)
            assert torch.equal(out2.view(-1), out)
    print("value head K=%d: worst |out - ref| / bound %.3f; relu(randn) rows: worst |out - ref| %.2f x 2^-24" % (K, worst, worst_plain))


def test_value_head_refuses_a_width_that_is_no_multiple_of_four_and_mismatched_tensors(eng):
    import torch
    from resource_packing_self_play_amd._lib import ERR_ARG, EngineError
    out = torch.full((5,), SENTINEL, device="cuda")
    for K in (2, 3, 6, 254):
        with pytest.raises(EngineError) as e:
            eng.nn_value_head(torch.ones((5, K), device="cuda"), torch.ones(K, device="cuda"), torch.zeros(1, device="cuda"), out)
        assert e.value.code == ERR_ARG
    z, w, b = torch.ones((5, 8), device="cuda"), torch.ones(8, device="cuda"), torch.zeros(1, device="cuda")
    bad_calls = [
        lambda: eng.nn_value_head(z, torch.ones(12, device="cuda"), b, out), lambda: eng.nn_value_head(z, w[:4], b, out),
        lambda: eng.nn_value_head(z, w, torch.zeros(2, device="cuda"), out), lambda: eng.nn_value_head(z, w, b, out[:4]),
        lambda: eng.nn_value_head(z, w, b, torch.empty(6, device="cuda")), lambda: eng.nn_value_head(z.double(), w, b, out),
        lambda: eng.nn_value_head(z, w.cpu(), b, out), lambda: eng.nn_value_head(z.t().contiguous().t(), w, b, out),
        lambda: eng.nn_value_head(z, torch.ones(16, device="cuda")[::2], b, out), lambda: eng.nn_value_head(z.view(5, 2, 4), w, b, out),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
