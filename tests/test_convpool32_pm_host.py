"""Host-side checks of the plan of the position-major 5x5 entry kernel (k_convpool32_pm): plan_convpool32 picks it for
32 -> 32 channels on 5x5 images where its cost rule says so, or where RP_CONVPOOL_PM forces it.  rp_debug_stage_plan keeps the knob at 0
(its recorded plans are k_convpool32's); rp_debug_convpool_plan exposes it (0: old kernel, 1: new kernel, -1: the cost rule).  No GPU needed."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "resource_packing_self_play_amd", "csrc", "librp_engine.so")
N_CU, LDS_PER_CU = 256, 160 * 1024
FAM_CP, FAM_CP_PM = 6, 8  # FAM_CP_PM is appended behind the families recorded in tests/golden/stage_plans.json
IMAGE_BYTES = 25 * 16 * 32 * 4  # [25 positions][16 leaves][32 floats]; the bias quads stay in registers
# rc, family, nt, waves, cin, tail, imgw, wave_floats, lds -- then grid, block
PM_PLAN = [0, FAM_CP_PM, 25, 4, 32, 0, 16, 0, IMAGE_BYTES]


@pytest.fixture(scope="module")
def plans():
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    i32, i64, out_t = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.rp_debug_stage_plan.argtypes = [i32, i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_convpool_plan.argtypes = [i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]

    def new(cin, B, H, W, cp_pm, n_cu=N_CU, lds=LDS_PER_CU, wgs=2, tail=1):
        out = (ctypes.c_int64 * 10)()
        rc = L.rp_debug_convpool_plan(cin, B, H, W, n_cu, lds, wgs, tail, cp_pm, out)
        return [rc] + list(out)

    def old(cin, B, H, W, n_cu=N_CU, lds=LDS_PER_CU, wgs=2, tail=1):
        out = (ctypes.c_int64 * 10)()
        rc = L.rp_debug_stage_plan(1, cin, B, H, W, n_cu, lds, wgs, tail, -1, out)
        return [rc] + list(out)
    return new, old


@pytest.mark.parametrize("B", (30000, 32768))
def test_cost_rule_picks_the_new_kernel_for_the_flagship_batches(plans, B):
    new, old = plans
    got = new(32, B, 5, 5, -1)
    assert got[:9] == PM_PLAN and got[10] == 256
    assert got[9] == min((B + 15) // 16, 2 * N_CU) and got[9] <= 512
    assert old(32, B, 5, 5)[1] == FAM_CP  # the recorded entry stays on k_convpool32


@pytest.mark.parametrize("B", (4096, 1030, 64, 1))
def test_cost_rule_keeps_the_old_kernel_for_small_batches(plans, B):
    new, old = plans
    got = new(32, B, 5, 5, -1)
    assert got[0] == 0 and got[1] == FAM_CP and got == old(32, B, 5, 5)


def test_cost_rule_figures_checked_by_hand(plans):
    """pm_rounds_cost(B, 16, 512) * 43 against pm_rounds_cost(B, imgw, 2048) * nt * 9, rounds(B) + 3 * rounds(0.92 B):
    32 768 rows: 16 * 43 = 688 < 21 * 45 = 945; 30 000: 688 < 20 * 45 = 900; 4 096: 4 * 43 = 172 > 4 * 36 = 144."""
    def cost(B, k, units):
        r = lambda rows: -(-(-(-rows // k)) // units)
        return r(B) + 3 * r(max(1, int(0.92 * B)))
    assert (cost(32768, 16, 512) * 43, cost(32768, 3, 2048) * 45) == (688, 945)
    assert (cost(30000, 16, 512) * 43, cost(30000, 3, 2048) * 45) == (688, 900)
    assert (cost(4096, 16, 512) * 43, cost(4096, 2, 2048) * 36) == (172, 144)
    new, _ = plans
    assert new(32, 4096, 5, 5, -1)[6] == 2 and new(32, 32768, 5, 5, 0)[6] == 3  # the leaves per wave the old costs above assume


def test_knob_forces_either_kernel_for_every_batch(plans):
    new, old = plans
    for B in (1, 2, 15, 16, 17, 64, 65, 1030, 4096, 8191, 8192, 8193, 30000, 32768, 100000, 1 << 22):
        got = new(32, B, 5, 5, 1)
        assert got[:9] == PM_PLAN and got[10] == 256 and got[9] == min((B + 15) // 16, 2 * N_CU), B
        assert new(32, B, 5, 5, 0) == old(32, B, 5, 5) and old(32, B, 5, 5)[1] == FAM_CP, B
    assert new(32, 0, 5, 5, 1) == [0] * 11  # nothing to launch


def test_other_shapes_keep_the_old_kernel_whatever_the_knob(plans):
    new, old = plans
    for (cin, H, W) in ((16, 5, 5), (32, 3, 3), (32, 4, 5), (32, 5, 4), (32, 6, 6), (16, 10, 10)):
        for B in (64, 30000):
            for knob in (1, -1):
                assert new(cin, B, H, W, knob) == old(cin, B, H, W), (cin, H, W, B, knob)
                assert new(cin, B, H, W, knob)[1] == FAM_CP


def test_workgroups_per_cu_follow_the_knob_and_the_lds(plans):
    new, _ = plans
    assert new(32, 32768, 5, 5, 1, wgs=3)[9] == 3 * N_CU     # three images fit 160 KB
    assert new(32, 32768, 5, 5, 1, wgs=4)[9] == 3 * N_CU     # a fourth does not
    assert new(32, 32768, 5, 5, 1, wgs=1)[9] == N_CU
    assert new(32, 32768, 5, 5, 1, lds=64 * 1024)[9] == N_CU  # 64 KB hold one image


def test_a_device_without_the_lds_never_gets_a_plan_it_cannot_hold(plans):
    new, old = plans
    for lds in (IMAGE_BYTES - 1, 48 * 1024, 32 * 1024, 16 * 1024, 4 * 1024):
        for knob in (1, -1):
            got = new(32, 32768, 5, 5, knob, lds=lds)
            assert got[1] != FAM_CP_PM and got[8] <= lds
            assert got == old(32, 32768, 5, 5, lds=lds)  # the old kernel, or its clean refusal (rc != 0, plan zeroed)
    assert new(32, 32768, 5, 5, 1, lds=IMAGE_BYTES)[1] == FAM_CP_PM


def test_knob_off_equals_the_recorded_entry_for_random_shapes(plans):
    new, old = plans
    rng = random.Random(20250)
    for _ in range(200):
        cin = rng.choice((16, 32))
        H, W = rng.randint(1, 40), rng.randint(1, 40)
        B = rng.choice((0, 1, rng.randint(1, 100), rng.randint(100, 10000), rng.randint(10000, 200000)))
        n_cu, lds = rng.choice(((256, 160 * 1024), (304, 64 * 1024), (104, 64 * 1024)))
        wgs, tail = rng.choice((1, 2, 3)), rng.choice((0, 1))
        assert new(cin, B, H, W, 0, n_cu, lds, wgs, tail) == old(cin, B, H, W, n_cu, lds, wgs, tail), (cin, B, H, W, n_cu, lds, wgs, tail)
