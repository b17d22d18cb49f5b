"""Host-side checks of the launch plan of the commit kernel's LDS-row mode (rp_commit_eval_logits_wide): the planner is plain
host code, reached through rp_debug_commit_plan.  It has to give every action space of the ABI a workgroup whose LDS the device can hand
out, account for every buffer the kernel lays out in it, and cover every slot.  No GPU needed."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "resource_packing_self_play_amd", "csrc", "librp_engine.so")
LDS_PER_CU = 160 * 1024
ACTIONS = (640, 1536, 1537, 1600, 6400, 8192)
SLOTS = (1, 5, 32768)
TERM_CHUNK = 1024  # floats of the term buffer: eight blocks of the pairwise sum


def n_leaves(n):
    """Blocks of NumPy's pairwise sum over n elements, as the engine's build_plan cuts them (<= 128 elements each, cuts at multiples of 8)."""
    if n <= 128:
        return 1
    n2 = n // 2
    n2 -= n2 % 8
    return n_leaves(n2) + n_leaves(n - n2)


@pytest.fixture(scope="module")
def plan():
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    L.rp_debug_commit_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.rp_debug_commit_plan.restype = ctypes.c_int

    def run(A, leaves, G, lds_per_cu=LDS_PER_CU):
        out = (ctypes.c_int64 * 8)()
        rc = L.rp_debug_commit_plan(A, leaves, G, lds_per_cu, out)
        return rc, dict(zip(("waves", "lds", "grid", "block", "row", "leaf", "term", "mask"), out))
    return run


@pytest.mark.parametrize("generous", [False, True], ids=["pairwise-plan", "128-leaves"])
@pytest.mark.parametrize("A", ACTIONS)
def test_lds_fits_the_device_and_holds_every_buffer(plan, A, generous):
    leaves = 128 if generous else n_leaves(A)
    rc, p = plan(A, leaves, 768)
    assert rc == 0
    assert p["waves"] in (1, 2, 4) and p["block"] == 64 * p["waves"]
    assert p["lds"] <= 160 * 1024
    # what the kernel lays out per wave: the row, one float64 per block, the term buffer, one mask bit per action
    assert p["row"] >= 4 * A and p["leaf"] >= 8 * leaves and p["term"] >= 4 * min(A, TERM_CHUNK) and p["mask"] >= 4 * ((A + 31) // 32)
    assert p["lds"] >= p["waves"] * (p["row"] + p["leaf"] + p["term"] + p["mask"])
    assert p["lds"] >= p["waves"] * A * 4 + p["waves"] * (8 * leaves + 4 * min(A, TERM_CHUNK) + 4 * ((A + 31) // 32))
    assert p["row"] % 16 == 0  # the kernel stores 16 bytes per lane into the row and puts the float64 block sums behind it


@pytest.mark.parametrize("A", ACTIONS)
def test_grid_covers_every_slot(plan, A):
    for G in SLOTS:
        rc, p = plan(A, n_leaves(A), G)
        assert rc == 0
        assert p["grid"] * p["waves"] >= G > (p["grid"] - 1) * p["waves"], (A, G, p)


@pytest.mark.parametrize("A", ACTIONS)
def test_shape_does_not_depend_on_the_slot_count(plan, A):
    shapes = {tuple(plan(A, n_leaves(A), G)[1][k] for k in ("waves", "lds", "block")) for G in SLOTS}
    assert len(shapes) == 1


def test_leaf_counts_follow_the_pairwise_rule():
    assert [n_leaves(a) for a in (128, 129, 640, 1536, 1600, 6400, 8192)] == [1, 2, 8, 16, 16, 64, 64]


def test_refusals(plan):
    assert plan(0, 1, 1)[0] == 1 and plan(8193, 64, 1)[0] == 1 and plan(640, 0, 1)[0] == 1 and plan(640, 129, 1)[0] == 1 and plan(640, 8, 0)[0] == 1
    rc, p = plan(8192, 64, 1, lds_per_cu=16 * 1024)  # a device that cannot hold one row: reported with the figures
    assert rc == 2 and p["lds"] > 16 * 1024
