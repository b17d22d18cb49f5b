"""Geometries, weights, float64 references and expected kernel routes of the fused evaluator (rp_leaf_stem ->
BinPackingNNet.forward_from_stem_fused with the engine as `ops`).  Host code only: test_evaluator_routes_cpu.py checks what is built
here and runs the glue on a pure-torch stand-in of the engine, test_gpu_evaluator_routes.py drives the kernels with it.

The states are leaf_inputs_ref.states(W, H, N): every one has a legal move, so every engine slot yields a leaf.  The weights follow a
seeded recipe that gives logits of order one (an untrained module's logits span ~1e-2, which hides a stage-level defect behind the
softmax).  Everything is computed in float64 on the CPU from those weights and cached: callers must not change what they get.

The accuracy bound of a geometry is 4 x its float32 noise floor -- the worst distance to the float64 truth of four float32 evaluations
of the SAME module through PyTorch on the CPU (floor() below), none of which runs the code under test.  The factor rests on the project's
own record: on one network, equally valid float32 summation orders land 0.5e-5 .. 4.0e-5 from the float64 truth (header of
test_gpu_nnet.py), a spread of 8 x, and a worst-of-four already sits in the upper part of that spread."""
import copy
import functools

import numpy as np

import leaf_inputs_ref as lir

# (W, H, N): stage images (16, 32, 32 channels) and what they reach
GEOMETRIES = [
    (64, 64, 12),  # 32x32, 16x16, 8x8: stage 0 on the library path (1024 px) with stem_relu; library entry conv + bias_pool NHWC4; then _wg and wave kernels
    (52, 49, 5),   # 25x26, 13x13, 7x7: first size over 640 (650 px); non-square
    (64, 40, 9),   # 20x32, 10x16, 5x8: exactly 640 px: k_resstage16_wg on 8 waves; Cin-16 entry at its limit
    (40, 30, 6),   # 15x20, 8x10, 4x5: 32-channel image of exactly 80 px (last wave-form size)
    (28, 16, 7),   # 8x14, 4x7, 2x4: 112 px: last wave-form size of the Cin-16 entry; 7 tiles
    (32, 16, 6),   # 8x16, 4x8, 2x4: 128 px: last wave-form size of k_resstage16; entry already _wg
    (12, 64, 65),  # 32x6, 16x3, 8x2: tall and narrow; second item word; A = 780
    (33, 8, 41),   # 4x17, 2x9, 1x5: first 64-bit row; item table in L2; a one-row last stage
    (64, 1, 3),    # 1x32, 1x16, 1x8: one-row images in every stage kernel
    (6, 5, 5),     # 3x3, 2x2, 1x1: dense-matrix sizes; a 1x1 image in rp_nn_resstage32
    (2, 3, 4),     # 2x1, 1x1, 1x1: one-column stem
    (1, 1, 1),     # 1x1 throughout: a 1x1 stem is both memory layouts at once
    (20, 20, 32),  # 10x10, 5x5, 3x3: production board (and the forced knobs, with 17 states)
]
CONFIGS = ("kernels", "cl", "nchw")  # what BatchedSelfPlay can select: channels-last with the stage kernels (production), channels-last
#                                      with resblock_kernel=False, channels_last=False
STATES = lir.STATES_PER_GEOMETRY
FORCED_GEOMETRY, FORCED_STATES = (20, 20, 32), 17  # 16-leaf tasks get a short second task, 8-leaf tasks a third
DRIVER_GEOMETRIES = [(52, 49, 5), (64, 40, 9), (6, 5, 5)]
SEED = 7
FACTOR = 4
STAGE16_MAX_PIXELS, STAGE32_MAX_PIXELS, DENSE_MAX_PIXELS = 640, 512, 9  # the documented limits (BinpackingNNet.py)
HIDDEN = 256


class Game:
    """What BinPackingNNet reads of a game (no engine behind it)."""

    def __init__(self, W, H, N):
        self.bin_width, self.bin_height, self.num_items = W, H, N

    def getBoardSize(self):
        return (self.bin_height, self.bin_width)

    def getActionSize(self):
        return self.bin_width * self.num_items


def images(geometry):
    """[(C, h, w)] of the stem (= stage 0's image) and of stages 1 and 2: the size halves rounding up."""
    W, H, _ = geometry
    out, h, w = [], H, W
    for ch in (16, 32, 32):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((ch, h, w))
    return out


def set_recipe_weights(module):
    """O(1) logits: walk named_parameters() in order with one CPU generator; a tensor with dim() > 1 gets randn * fan ** -0.5,
    fan = p[0].numel(), a bias 0.1 * randn.  Works on a module on any device (the numbers are drawn on the CPU)."""
    import torch
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        for _, p in module.named_parameters():
            r = torch.randn(p.shape, generator=g, dtype=torch.float32)
            r = r * float(p[0].numel()) ** -0.5 if p.dim() > 1 else 0.1 * r
            p.copy_(r.to(p.device))
    return module


def make_module(geometry):
    """A fresh float32 BinPackingNNet on the CPU with the recipe's weights, in eval mode."""
    import torch
    from resource_packing_self_play_amd.binpacking.pytorch.BinpackingNNet import BinPackingNNet
    from resource_packing_self_play_amd.utils import dotdict
    W, H, N = geometry
    with torch.random.fork_rng(devices=[]):
        net = BinPackingNNet(Game(W, H, N), dotdict(num_items=N, num_bins=1))
    return set_recipe_weights(net).eval()


def states(geometry, count=STATES):
    return lir.states(*geometry, count=count)


@functools.lru_cache(maxsize=None)
def _planes(geometry, count):
    import torch
    return torch.from_numpy(states(geometry, count).planes())  # float32 zeros and ones: exact in every format


def _forward64(net64, x64, hooked_stage=None):
    """(logits, v, first layer) of the float64 module; hooked_stage: that stage's output gets out[:, 3, -1, -1] = 0."""
    import torch
    import torch.nn.functional as F
    handle = None
    if hooked_stage is not None:
        def hook(_module, _inputs, out):
            out = out.clone()
            out[:, 3, -1, -1] = 0.0
            return out
        handle = net64.conv_seqs[hooked_stage].register_forward_hook(hook)
    try:
        with torch.no_grad():
            z = net64.trunk(x64)
            logits, v = net64.logits_fc(z), torch.tanh(net64.value_fc(z))
            y = F.max_pool2d(net64.conv_seqs[0].conv(x64), 3, 2, 1)
    finally:
        if handle is not None:
            handle.remove()
    return logits, v, y


@functools.lru_cache(maxsize=None)
def _truth(geometry, count):
    net64 = copy.deepcopy(make_module(geometry)).double()
    logits, v, y = _forward64(net64, _planes(geometry, count).double())
    return logits, v, y


def truth(geometry, count=STATES):
    """(logits64 [S, A], v64 [S]) of the float64 deep copy of the module on States.planes(); v64 = tanh(value_fc(z))."""
    logits, v, _ = _truth(geometry, count)
    out = logits.numpy().copy(), v.numpy().reshape(-1).copy()
    for a in out:
        a.setflags(write=False)
    return out


def _raw32(net, z_of):
    """(logits, v) as float64 numpy from a float32 trunk output."""
    import torch
    with torch.no_grad():
        z = z_of()
        return net.logits_fc(z).double().numpy(), torch.tanh(net.value_fc(z)).double().numpy().reshape(-1)


def _from_stem_raw(net, y):
    """forward_from_stem without the log-softmax: (logits, v) float64 numpy."""
    import torch
    import torch.nn.functional as F

    def z():
        st0 = net.conv_seqs[0]
        t = st0.res_block1(st0.res_block0(y))
        for stage in net.conv_seqs[1:]:
            t = stage(t)
        return F.relu(net.hidden_fc(F.relu(torch.flatten(t, start_dim=1))))
    return _raw32(net, z)


@functools.lru_cache(maxsize=None)
def _floor(geometry, count):
    import torch
    W, H, N = geometry
    net = make_module(geometry)
    x = _planes(geometry, count)
    logits64, v64, y64 = _truth(geometry, count)
    logits64, v64 = logits64.numpy(), v64.numpy().reshape(-1)
    evals = {"batch": _raw32(net, lambda: net.trunk(x))}
    one = [_raw32(net, lambda k=k: net.trunk(x[k:k + 1])) for k in range(len(x))]
    evals["one by one"] = (np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one]))
    net_cl = copy.deepcopy(net).to(memory_format=torch.channels_last)
    evals["channels-last"] = _raw32(net_cl, lambda: net_cl.trunk(x.contiguous(memory_format=torch.channels_last)))
    # behind a first layer that is as good as the stem's contract allows: the exact one rounded to float32, every element then moved by
    # +- its stem_tolerance
    conv = net.conv_seqs[0].conv
    Bq, q = lir.stem_bound(conv.weight.detach().numpy(), conv.bias.detach().numpy(), N)
    y = y64.numpy()
    tol = lir.stem_tolerance(Bq, q, N, y, y)
    sign = np.random.default_rng([SEED, W, H, N, count]).integers(0, 2, y.shape) * 2.0 - 1.0
    moved = torch.from_numpy((y.astype(np.float32).astype(np.float64) + sign * tol).astype(np.float32))
    evals["moved stem"] = _from_stem_raw(net, moved)
    gaps = {k: (float(np.abs(lg - logits64).max()), float(np.abs(v - v64).max())) for k, (lg, v) in evals.items()}
    return max(g[0] for g in gaps.values()), max(g[1] for g in gaps.values()), gaps


def floor(geometry, count=STATES):
    """(logit floor, v floor): the worst |out32 - out64| over four CPU float32 evaluations of the module -- the whole batch, one state
    at a time, module and input in channels-last, and forward_from_stem behind the float64 first layer rounded to float32 and moved
    by +- leaf_inputs_ref.stem_tolerance (the stem's own accuracy contract) with seeded random signs."""
    return _floor(geometry, count)[:2]


def floor_parts(geometry, count=STATES):
    """{variant: (logit gap, v gap)} behind floor()."""
    return dict(_floor(geometry, count)[2])


def bound(geometry, count=STATES):
    """(logit bound, v bound) = FACTOR x floor."""
    fl, fv = floor(geometry, count)
    return FACTOR * fl, FACTOR * fv


@functools.lru_cache(maxsize=None)
def mutations(geometry, count=STATES):
    """Per stage, the largest logit change over the batch when that stage's output gets out[:, 3, -1, -1] = 0 in the float64 forward (a
    one-pixel, one-channel defect; the largest over the batch because some states have that unit dead behind the ReLU)."""
    net64 = copy.deepcopy(make_module(geometry)).double()
    x64 = _planes(geometry, count).double()
    base = _truth(geometry, count)[0]
    return tuple(float((_forward64(net64, x64, hooked_stage=si)[0] - base).abs().max()) for si in range(3))


def logit_span(geometry, count=STATES):
    """How far the geometry's float64 logits reach from zero: the largest |logit|.  (Not a difference between logits: (1, 1, 1) has one
    action and one possible state, so all its logits are one number.)  The recipe gives 0.19 at (2, 3, 4) to 3.3 at (32, 16, 6)."""
    return float(_truth(geometry, count)[0].abs().max())


# ---- routes ------------------------------------------------------------------------------------------------------------------------
def route_is_channels_last(geometry, config):
    """A 1x1 stem is contiguous in both layouts, so BinPackingNNet._is_cl reports NCHW: (1, 1, 1) takes the NCHW library route in
    every config."""
    _, h, w = images(geometry)[0]
    return config != "nchw" and h * w > 1


def expected_route(geometry, config, fused_linear_relu=True):
    """[stage 0, stage 1, stage 2, head], each the ordered list of (op name, C, H, W, channels_last) of the `ops` calls the evaluator
    must make; (C, H, W) is the shape of the call's first tensor and channels_last says whether that tensor is channels-last and NOT
    NCHW-contiguous (a 1x1 image is both, and counts as NCHW).  Written from the documented limits alone: a stage runs on its stage
    kernel when the route is channels-last with the stage kernels and its image has at most 640 (16 channels) / 512 (32 channels)
    pixels; a 32-channel stage is entered through the entry kernel when the PREVIOUS stage's image fits that stage's limit; everything
    else is the library path (convolution, or a dense matrix up to DENSE_MAX_PIXELS pixels, between the element-wise kernels).
    fused_linear_relu: the hidden layer's bias + ReLU is the GEMM's epilogue (BinPackingNNet.fused_linear_relu), else one more
    nn_bias_relu."""
    cl = route_is_channels_last(geometry, config)
    kern = cl and config == "kernels"
    limit = {16: STAGE16_MAX_PIXELS, 32: STAGE32_MAX_PIXELS}
    img = images(geometry)
    route = []
    for si, (ch, h, w) in enumerate(img):
        calls = []
        if si > 0:
            pc, ph, pw = img[si - 1]
            if kern and ph * pw <= limit[pc]:
                calls.append(("nn_convpool32", pc, ph, pw, cl and ph * pw > 1))
            else:
                calls.append(("nn_bias_pool", ch, ph, pw, cl and ph * pw > 1))
        flag = cl and h * w > 1
        if kern and h * w <= limit[ch]:
            calls.append(("nn_resstage%d" % ch, ch, h, w, flag))
        else:
            calls += [("nn_bias_relu", ch, h, w, flag), ("nn_bias_residual", ch, h, w, flag)] * 2
        route.append(calls)
    head = [] if fused_linear_relu else [("nn_bias_relu", HIDDEN, 1, 1, False)]
    route.append(head + [("nn_value_head", HIDDEN, 1, 1, False)])
    return route


def flat(route):
    return [c for stage in route for c in stage]


def stage0_on_kernel(geometry, config):
    return expected_route(geometry, config)[0][0][0] == "nn_resstage16"


def passes_stem_relu(geometry, config):
    """BatchedSelfPlay allocates stem_relu unless stage 0 runs on the stage kernel: its own copy of the 640-pixel rule
    (selfplay.py, stage0_kernel) asks the configuration and the image size only, not the layout."""
    _, h, w = images(geometry)[0]
    return not (config == "kernels" and h * w <= STAGE16_MAX_PIXELS)


def is_channels_last(t):
    """BinPackingNNet._is_cl's rule, for the recorders."""
    import torch
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def describe(name, t):
    """The record of one `ops` call from its first tensor."""
    h, w = (int(t.shape[2]), int(t.shape[3])) if t.dim() == 4 else (1, 1)
    return (name, int(t.shape[1]), h, w, bool(is_channels_last(t)))


class Recorder:
    """Proxy around an `ops` object (the engine): records describe() of every nn_* call and passes it on."""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)  # AttributeError where the engine has none: hasattr(ops, "nn_value_head") stays truthful
        if not name.startswith("nn_"):
            return fn

        def call(x, *args, **kw):
            self.calls.append(describe(name, x))
            return fn(x, *args, **kw)
        return call


class TorchOps:
    """Pure-torch stand-in for the engine's nn_* methods on the CPU; records describe() of every call but the weight packers.  The
    packers copy the flat weight into the fragment buffer (the buffers hold exactly a weight's elements), the stage and entry stand-ins
    reshape it back.  Like the engine, every call refuses tensors that are not all in one memory order."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _one_order(what, *tensors):
        import torch
        orders = {"nchw", "nhwc"}
        for t in tensors:
            if t is None:
                continue
            mine = {"nchw"} if t.is_contiguous() else set()
            if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
                mine.add("nhwc")
            orders &= mine
        if not orders:
            raise ValueError("%s: tensors in different memory orders" % what)

    @staticmethod
    def _needs_cl(what, x, channels):
        import torch
        if x.dim() != 4 or x.shape[1] != channels or not x.is_contiguous(memory_format=torch.channels_last):
            raise ValueError("%s needs a channels-last [B, %d, H, W] tensor" % (what, channels))

    def nn_pack_conv16(self, weight, frag):
        assert tuple(weight.shape) == (16, 16, 3, 3) and weight.is_contiguous() and frag.numel() == weight.numel()
        frag.copy_(weight.reshape(-1))

    def nn_pack_conv32(self, weight, frag):
        assert weight.shape[0] == 32 and weight.shape[1] in (16, 32) and weight.is_contiguous() and frag.numel() == weight.numel()
        frag.copy_(weight.reshape(-1))

    def _resstage(self, name, ch, x, frag4, bias4, out, out_relu):
        import torch
        import torch.nn.functional as F
        self._needs_cl(name, x, ch)
        self._one_order(name, x, out, out_relu)
        self.calls.append(describe(name, x))
        n = ch * ch * 9
        assert frag4.numel() == 4 * n and bias4.numel() == 4 * ch
        w = [frag4[k * n:(k + 1) * n].view(ch, ch, 3, 3) for k in range(4)]
        b = [bias4[k * ch:(k + 1) * ch] for k in range(4)]
        t = x
        for k in (0, 2):
            y = F.conv2d(torch.relu(t), w[k], b[k], padding=1)
            t = F.conv2d(torch.relu(y), w[k + 1], b[k + 1], padding=1) + t
        out.copy_(t)
        if out_relu is not None:
            out_relu.copy_(torch.relu(t))

    def nn_resstage16(self, x, frag4, bias4, out, out_relu=None):
        if x.shape[2] * x.shape[3] > STAGE16_MAX_PIXELS:
            raise ValueError("nn_resstage16: more than 640 pixels")
        self._resstage("nn_resstage16", 16, x, frag4, bias4, out, out_relu)

    def nn_resstage32(self, x, frag4, bias4, out, out_relu=None):
        if x.shape[2] * x.shape[3] > STAGE32_MAX_PIXELS:
            raise ValueError("nn_resstage32: more than 512 pixels")
        self._resstage("nn_resstage32", 32, x, frag4, bias4, out, out_relu)

    def nn_convpool32(self, x, frag, bias, out):
        import torch.nn.functional as F
        cin = int(x.shape[1])
        self._needs_cl("nn_convpool32", x, cin)
        self._needs_cl("nn_convpool32", out, 32)
        if cin not in (16, 32) or x.shape[2] * x.shape[3] > (STAGE16_MAX_PIXELS if cin == 16 else STAGE32_MAX_PIXELS):
            raise ValueError("nn_convpool32: bad shape")
        self.calls.append(describe("nn_convpool32", x))
        assert frag.numel() == 32 * cin * 9
        out.copy_(F.max_pool2d(F.conv2d(x, frag.view(32, cin, 3, 3), bias, padding=1), 3, 2, 1))

    def nn_bias_relu(self, x, bias):
        import torch
        self._one_order("nn_bias_relu", x)
        self.calls.append(describe("nn_bias_relu", x))
        x.copy_(torch.relu(x + bias.view(1, -1, 1, 1)))
        return x

    def nn_bias_residual(self, x, bias, res, out, out_relu=None):
        import torch
        self._one_order("nn_bias_residual", x, res, out, out_relu)
        self.calls.append(describe("nn_bias_residual", x))
        out.copy_((x + bias.view(1, -1, 1, 1)) + res)
        if out_relu is not None:
            out_relu.copy_(torch.relu(out))

    def nn_bias_pool(self, x, bias, out, out_relu=None):
        import torch
        import torch.nn.functional as F
        self._one_order("nn_bias_pool", x, out, out_relu)
        self.calls.append(describe("nn_bias_pool", x))
        out.copy_(F.max_pool2d(x + bias.view(1, -1, 1, 1), 3, 2, 1))
        if out_relu is not None:
            out_relu.copy_(torch.relu(out))

    def nn_value_head(self, z, weight, bias, out):
        import torch
        self.calls.append(describe("nn_value_head", z))
        out.copy_(torch.tanh(z @ weight.reshape(-1, 1) + bias).reshape(out.shape))


def configure(module, config):
    """The module in the config's memory format with the config's kernel switch, its caches empty."""
    import torch
    module.to(memory_format=torch.contiguous_format if config == "nchw" else torch.channels_last)
    module.use_resblock_kernel = config == "kernels"
    if hasattr(module, "_dense"):
        module._dense.clear()
    return module


def gaps(logits, v, geometry, count=STATES, rows=None):
    """(largest |logits - logits64|, largest |v - v64|, largest |softmax(logits) - softmax(logits64)|) at the truth's rows `rows`."""
    logits64, v64 = truth(geometry, count)
    if rows is not None:
        logits64, v64 = logits64[rows], v64[rows]
    logits = np.asarray(logits, np.float64)

    def softmax(x):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return (float(np.abs(logits - logits64).max()), float(np.abs(np.asarray(v, np.float64).reshape(-1) - v64).max()),
            float(np.abs(softmax(logits) - softmax(logits64)).max()))
