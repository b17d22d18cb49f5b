"""The fused evaluator's references, routes and glue without a GPU (evaluator_routes_ref.py): conditions the float64 reference and
its bound must meet for test_gpu_evaluator_routes.py to mean anything, what the expected routes cover, which kernel families the stage
planners pick at the batch sizes the GPU test uses, and BinPackingNNet.forward_from_stem_fused itself on a pure-torch stand-in of the
engine."""
import ctypes
import os

import numpy as np
import pytest

import evaluator_routes_ref as err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "resource_packing_self_play_amd", "csrc", "librp_engine.so")
N_CU, LDS_PER_CU = 256, 160 * 1024
# rp_engine.hip's family enumeration (FAM_*), in order
FAMILIES = ["none", "k_resstage16", "k_resstage16_wg", "k_resstage32", "k_resstage32_wg", "k_resstage32_pm", "k_convpool32", "k_convpool32_wg",
            "k_convpool32_pm", "k_resstage16_pp"]
GEOMETRY_IDS = ["%dx%d-%d" % g for g in err.GEOMETRIES]


# ---- the reference alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", err.GEOMETRIES, ids=GEOMETRY_IDS)
def test_floor_is_finite_and_positive(geometry):
    fl, fv = err.floor(geometry)
    print("%r floor: logits %.3e v %.3e  %r" % (geometry, fl, fv, err.floor_parts(geometry)))
    assert np.isfinite(fl) and np.isfinite(fv) and fl > 0.0 and fv > 0.0


@pytest.mark.parametrize("geometry", err.GEOMETRIES, ids=GEOMETRY_IDS)
def test_bound_cannot_hide_a_one_pixel_defect_in_any_stage(geometry):
    """Zeroing one corner pixel of one channel of a stage's output moves a logit by at least 10 x the bound (smallest ratio on record:
    about 170, stage 0 of (64, 64, 12): 1.3e-3 against 4 x 2.0e-6)."""
    b, _ = err.bound(geometry)
    mu = err.mutations(geometry)
    print("%r bound %.3e mutations %s" % (geometry, b, " ".join("%.3e" % m for m in mu)))
    for si, m in enumerate(mu):
        assert m >= 10.0 * b, "stage %d: a one-pixel defect moves the logits by %.3e, the bound is %.3e" % (si, m, b)


@pytest.mark.parametrize("geometry", err.GEOMETRIES, ids=GEOMETRY_IDS)
def test_logits_are_of_order_one(geometry):
    assert err.logit_span(geometry) >= 0.1


def test_forced_knob_states_meet_the_same_conditions():
    g, n = err.FORCED_GEOMETRY, err.FORCED_STATES
    b, _ = err.bound(g, n)
    assert len(err.states(g, n)) == n and 0.0 < b < np.inf
    assert min(err.mutations(g, n)) >= 10.0 * b and err.logit_span(g, n) >= 0.1


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
def _routes():
    return {(g, c): err.expected_route(g, c) for g in err.GEOMETRIES for c in err.CONFIGS}


def test_routes_contain_every_op_kind_in_every_layout_it_can_have():
    calls = {c for r in _routes().values() for c in err.flat(r)}
    kinds = {(name, cl) for (name, _, _, _, cl) in calls}
    for name in ("nn_bias_relu", "nn_bias_residual", "nn_bias_pool"):  # the library path runs in both layouts
        assert (name, True) in kinds and (name, False) in kinds
    for name in ("nn_resstage16", "nn_resstage32", "nn_convpool32"):  # channels-last only (a 1x1 image is both and counts as NCHW)
        assert (name, True) in kinds
    assert {ch for (name, ch, _, _, _) in calls if name == "nn_convpool32"} == {16, 32}
    assert ("nn_value_head", False) in kinds
    # <= 9-pixel images on the library path (the dense matrices) in both layouts, and larger ones (the library convolution)
    small = {cl for (name, _, h, w, cl) in calls if name == "nn_bias_residual" and 1 < h * w <= err.DENSE_MAX_PIXELS}
    large = {cl for (name, _, h, w, cl) in calls if name == "nn_bias_residual" and h * w > err.DENSE_MAX_PIXELS}
    assert small == {True, False} and large == {True, False}


def test_production_routes_cross_every_routing_limit():
    routes = {g: err.expected_route(g, "kernels") for g in err.GEOMETRIES}
    names = lambda stage: [c[0] for c in stage]
    library = ["nn_bias_relu", "nn_bias_residual"] * 2
    # stage 0 on the library path, stage kernels from stage 1 on, entered through nn_bias_pool
    for g in ((64, 64, 12), (52, 49, 5)):
        r = routes[g]
        assert names(r[0]) == library and names(r[1]) == ["nn_bias_pool", "nn_resstage32"] and names(r[2]) == ["nn_convpool32", "nn_resstage32"]
        assert not err.stage0_on_kernel(g, "kernels") and err.passes_stem_relu(g, "kernels")
    assert routes[(52, 49, 5)][0][0][2:4] == (25, 26) and 25 * 26 == err.STAGE16_MAX_PIXELS + 10
    calls = {c for r in routes.values() for c in err.flat(r)}
    for call in [("nn_resstage16", 16, 20, 32, True), ("nn_convpool32", 16, 20, 32, True),   # exactly 640 pixels
                 ("nn_resstage32", 32, 8, 10, True), ("nn_convpool32", 32, 8, 10, True),      # exactly 80
                 ("nn_resstage16", 16, 8, 14, True), ("nn_convpool32", 16, 8, 14, True),      # 112
                 ("nn_resstage16", 16, 8, 16, True), ("nn_convpool32", 16, 8, 16, True),      # 128
                 ("nn_resstage16", 16, 1, 32, True), ("nn_convpool32", 32, 1, 16, True), ("nn_resstage32", 32, 1, 8, True),  # one-row images
                 ("nn_resstage32", 32, 1, 5, True), ("nn_resstage16", 16, 2, 1, True),        # a one-row last stage, a one-column stem
                 ("nn_resstage32", 32, 1, 1, False), ("nn_convpool32", 32, 1, 1, False),      # 1x1 images in the stage kernels
                 ("nn_resstage16", 16, 3, 3, True), ("nn_resstage32", 32, 2, 2, True),        # dense-matrix sizes on the stage kernels
                 ("nn_resstage16", 16, 10, 10, True), ("nn_convpool32", 32, 5, 5, True), ("nn_resstage32", 32, 3, 3, True)]:  # production
        assert call in calls, call
    # the 1x1 stem: the NCHW library route in every config
    for c in err.CONFIGS:
        assert err.expected_route((1, 1, 1), c) == err.expected_route((1, 1, 1), "nchw")
        assert all(not call[4] and not call[0].startswith(("nn_resstage", "nn_convpool")) for call in err.flat(err.expected_route((1, 1, 1), c)))


def test_both_copies_of_the_640_pixel_rule_agree_wherever_the_route_is_channels_last():
    """BatchedSelfPlay hands the evaluator no stem_relu when its own copy of the rule says that stage 0 runs on the stage kernel.  The two
    copies differ only at the 1x1 stem, where the library route takes relu(stem) itself."""
    for g in err.GEOMETRIES:
        for c in err.CONFIGS:
            if g == (1, 1, 1) and c == "kernels":
                assert not err.stage0_on_kernel(g, c) and not err.passes_stem_relu(g, c)
            else:
                assert err.passes_stem_relu(g, c) == (not err.stage0_on_kernel(g, c))


# ---- planner families ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    i32, i64, out_t = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.rp_debug_stage_plan.argtypes = [i32, i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_convpool_plan.argtypes = [i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_stage16_plan.argtypes = [i64, i32, i32, i32, i64, i32, i32, i32, out_t]

    def run(call, B, knob=-1):
        """(family name, waves, Cin) of the launch behind one route entry; knob: the entry point's RP_STAGE16_PP / RP_CONVPOOL_PM /
        RP_STAGE32_PM (-1: unset, the cost rule)."""
        name, ch, h, w, _ = call
        out = (ctypes.c_int64 * 10)()
        if name == "nn_resstage16":
            rc = L.rp_debug_stage16_plan(B, h, w, N_CU, LDS_PER_CU, 2, 1, knob, out)
        elif name == "nn_convpool32":
            rc = L.rp_debug_convpool_plan(ch, B, h, w, N_CU, LDS_PER_CU, 2, 1, knob, out)
        else:
            rc = L.rp_debug_stage_plan(2, 32, B, h, w, N_CU, LDS_PER_CU, 2, 1, knob, out)
        assert rc == 0 and out[5] >= 1, call
        return FAMILIES[out[0]], int(out[2]), int(out[3])
    return run


def _stage_calls(geometry):
    return [c for c in err.flat(err.expected_route(geometry, "kernels")) if c[0].startswith(("nn_resstage", "nn_convpool"))]


def test_table_geometries_reach_every_pixel_major_family(plan):
    reached = {plan(c, err.STATES) for g in err.GEOMETRIES for c in _stage_calls(g)}
    print(sorted(reached))
    want = {("k_resstage16", 4, 16), ("k_resstage16_wg", 4, 16), ("k_resstage16_wg", 8, 16), ("k_resstage32", 4, 32),
            ("k_convpool32", 4, 16), ("k_convpool32", 4, 32), ("k_convpool32_wg", 16), ("k_convpool32_wg", 32), ("k_resstage32_wg",)}
    got = reached | {(f, cin) for (f, _, cin) in reached} | {(f,) for (f, _, _) in reached}
    assert want <= got, sorted(want - got)
    # the boundary sizes sit on the side of the limit the table says
    assert plan(("nn_resstage16", 16, 20, 32, True), err.STATES) == ("k_resstage16_wg", 8, 16)
    assert plan(("nn_resstage16", 16, 8, 16, True), err.STATES)[0] == "k_resstage16" and plan(("nn_convpool32", 16, 8, 16, True), err.STATES)[0] == "k_convpool32_wg"
    assert plan(("nn_convpool32", 16, 8, 14, True), err.STATES)[0] == "k_convpool32"
    assert plan(("nn_resstage32", 32, 8, 10, True), err.STATES)[0] == "k_resstage32" and plan(("nn_convpool32", 32, 8, 10, True), err.STATES)[0] == "k_convpool32"
    # at this batch size the cost rules keep the pixel-major kernels on the production board: the newer ones need the forced knobs
    assert {plan(c, err.FORCED_STATES)[0] for c in _stage_calls(err.FORCED_GEOMETRY)} == {"k_resstage16", "k_convpool32", "k_resstage32"}


def test_forced_knobs_select_the_newer_kernels_on_the_production_board(plan):
    calls = _stage_calls(err.FORCED_GEOMETRY)
    assert [c[:4] for c in calls] == [("nn_resstage16", 16, 10, 10), ("nn_convpool32", 16, 10, 10), ("nn_resstage32", 32, 5, 5),
                                      ("nn_convpool32", 32, 5, 5), ("nn_resstage32", 32, 3, 3)]
    on = [plan(c, err.FORCED_STATES, 1)[0] for c in calls]
    off = [plan(c, err.FORCED_STATES, 0)[0] for c in calls]
    assert on == ["k_resstage16_pp", "k_convpool32", "k_resstage32_pm", "k_convpool32_pm", "k_resstage32_pm"]  # the Cin-16 entry has no newer form
    assert off == ["k_resstage16", "k_convpool32", "k_resstage32", "k_convpool32", "k_resstage32"]


# ---- the glue on the CPU ---------------------------------------------------------------------------------------------------------------
def run_glue(geometry, config, count=err.STATES):
    """forward_from_stem_fused with TorchOps, fed the float32 module's own first layer -> (logits, v, recorded calls, module)."""
    import torch
    import torch.nn.functional as F
    net = err.configure(err.make_module(geometry), config)
    ops = err.TorchOps()
    net.refresh_dense()
    keep = net.refresh_frags(ops) if config == "kernels" else None
    x = torch.from_numpy(err.states(geometry, count).planes())
    fmt = torch.contiguous_format if config == "nchw" else torch.channels_last
    with torch.no_grad():
        y = F.max_pool2d(net.conv_seqs[0].conv(x), 3, 2, 1).contiguous(memory_format=fmt)
        y_relu = torch.relu(y) if err.passes_stem_relu(geometry, config) else None
        logits, v = net.forward_from_stem_fused(y, y_relu, ops, logits=True)
    del keep
    return logits.numpy(), v.numpy().reshape(-1), ops.calls, net


@pytest.mark.parametrize("config", err.CONFIGS)
@pytest.mark.parametrize("geometry", err.GEOMETRIES, ids=GEOMETRY_IDS)
def test_glue_on_torch_ops_matches_truth_and_takes_the_expected_route(geometry, config):
    logits, v, calls, net = run_glue(geometry, config)
    want = err.expected_route(geometry, config, net.fused_linear_relu)
    assert calls == err.flat(want), "route differs:\n got %r\nwant %r" % (calls, err.flat(want))
    gl, gv, gs = err.gaps(logits, v, geometry)
    (bl, bv), (fl, fv) = err.bound(geometry), err.floor(geometry)
    print("%r %s: |logits - f64| %.3e (floor %.3e) |v - f64| %.3e (floor %.3e)" % (geometry, config, gl, fl, gv, fv))
    assert gl <= bl and gv <= bv
    dense = set(getattr(net, "_dense", {}))
    img = err.images(geometry)
    for si, (_, h, w) in enumerate(img):  # the dense matrices exist exactly for the <= 9-pixel stages
        assert ("%d:b0c0" % si in dense) == (h * w <= err.DENSE_MAX_PIXELS) and ("%d:b1c1:cl" % si in dense) == (h * w <= err.DENSE_MAX_PIXELS)
    limit = {16: err.STAGE16_MAX_PIXELS, 32: err.STAGE32_MAX_PIXELS}
    for si, (ch, h, w) in enumerate(img):  # refresh_frags packs what the limits allow, whatever the route later takes
        assert ("stagefrag:%d" % si in dense) == (config == "kernels" and h * w <= limit[ch])
        if si > 0:
            pc, ph, pw = img[si - 1]
            assert ("entryfrag:%d" % si in dense) == (config == "kernels" and ph * pw <= limit[pc])


def test_glue_detects_a_one_pixel_defect_in_a_stage_kernel():
    """The check itself: a stand-in whose 16-channel stage kernel zeroes one corner pixel of one channel misses the bound."""
    import torch
    g = (64, 40, 9)

    class Broken(err.TorchOps):
        def nn_resstage16(self, x, frag4, bias4, out, out_relu=None):
            super().nn_resstage16(x, frag4, bias4, out, out_relu)
            out[:, 3, -1, -1] = 0.0
            if out_relu is not None:
                out_relu[:, 3, -1, -1] = 0.0

    net = err.configure(err.make_module(g), "kernels")
    ops = Broken()
    net.refresh_dense()
    keep = net.refresh_frags(ops)
    x = torch.from_numpy(err.states(g).planes())
    with torch.no_grad():
        y = torch.nn.functional.max_pool2d(net.conv_seqs[0].conv(x), 3, 2, 1).contiguous(memory_format=torch.channels_last)
        logits, v = net.forward_from_stem_fused(y, None, ops, logits=True)
    del keep
    gl, _, gs = err.gaps(logits.numpy(), v.numpy(), g)
    assert gl > 10.0 * err.bound(g)[0]
    print("one-pixel defect: |logits - f64| %.3e, bound %.3e; softmax moves by %.3e" % (gl, err.bound(g)[0], gs))
