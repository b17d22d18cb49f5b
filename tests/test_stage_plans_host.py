"""Host-side checks of the launch plans of the CNN stage kernels: the planners behind rp_nn_resstage16 /
rp_nn_convpool32 / rp_nn_resstage32 are plain host code, reached here through rp_debug_stage_plan.  tests/golden/stage_plans.json holds
what the launchers of the commit before the planners did at every launch site (kernel family and template arguments, leaves per wave
or workgroup, LDS bytes, grid, block), for explicit rows and as one digest per entry point over all images up to 40 x 40.  No GPU needed."""
import ctypes
import hashlib
import json
import os

import pytest

import stage_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "resource_packing_self_play_amd", "csrc", "librp_engine.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_plans.json")
RESSTAGE16, CONVPOOL32, RESSTAGE32 = 0, 1, 2  # rp_debug_stage_plan's entry
# every instantiation of every launch table in rp_engine.hip: (family, nt, waves, cin, tail blocks)
TABLES = ([("k_resstage16", nt, 4, 16, 0) for nt in range(1, 9)] + [("k_resstage16", 6, 4, 16, 1)]
          + [("k_resstage16_wg", nt, wv, 16, 0) for wv in (4, 8) for nt in (3, 4, 5)]
          + [("k_resstage32", nt, 4, 32, 0) for nt in range(1, 6)]
          + [("k_resstage32_wg", nt, wv, 32, 0) for (nt, wv) in ((2, 4), (3, 4), (4, 4), (3, 8), (4, 8))]
          + [("k_resstage32_pm", s * s, 4, 32, 0) for s in (3, 5)]
          + [("k_convpool32", nt, 4, 16, 0) for nt in range(1, 8)] + [("k_convpool32", 6, 4, 16, 1)] + [("k_convpool32", nt, 4, 32, 0) for nt in range(1, 6)]
          + [("k_convpool32_wg", nt, wv, 16, 0) for (nt, wv) in ((2, 4), (3, 4), (4, 4), (3, 8), (4, 8), (5, 8))]
          + [("k_convpool32_wg", nt, wv, 32, 0) for (nt, wv) in ((2, 4), (3, 4), (4, 4), (3, 8), (4, 8))])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plan(golden):
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    L.rp_debug_stage_plan.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    devices = [(d["n_cu"], d["lds_per_cu"]) for d in golden["devices"]]

    def run(entry, cin, B, H, W, device=0, wgs=2, tail=1, pm_force=-1):
        out = (ctypes.c_int64 * 10)()
        rc = L.rp_debug_stage_plan(entry, cin, B, H, W, devices[device][0], devices[device][1], wgs, tail, pm_force, out)
        return [rc] + list(out)
    return run


def test_every_recorded_launch_is_reproduced(golden, plan):
    assert golden["columns"][:10] == ["entry", "Cin", "B", "H", "W", "device", "wgs", "tail", "pm_force", "rc"] and len(golden["rows"]) > 1000
    wrong = [(row[:9], row[9:], plan(*row[:9])) for row in golden["rows"] if plan(*row[:9]) != row[9:]]
    assert not wrong, "%d of %d plans differ, first (inputs, recorded, now): %r" % (len(wrong), len(golden["rows"]), wrong[0])
    assert {row[9] for row in golden["rows"]} == {0, 1, 2} and {row[10] for row in golden["rows"]} >= set(range(1, 8))  # every return, every family


@pytest.mark.parametrize("name,entry,cins,limit", [("resstage16", RESSTAGE16, (16,), 640), ("convpool32", CONVPOOL32, (16, 32), (640, 512)),
                                                   ("resstage32", RESSTAGE32, (32,), 512)])
def test_sweep_over_all_images_up_to_40x40_matches_the_recorded_digest(golden, plan, name, entry, cins, limit):
    sweep = golden["sweep"]
    limits = dict(zip(cins, limit if isinstance(limit, tuple) else (limit,)))
    h, n = hashlib.sha256(), 0
    for cin in cins:
        for H in range(1, 41):
            for W in range(1, 41):
                if H * W > limits[cin]:
                    continue
                for B in sweep["batches"]:
                    h.update((" ".join(str(v) for v in [cin, B, H, W] + plan(entry, cin, B, H, W)) + "\n").encode())
                    n += 1
    assert n == sweep["digests"][name]["cases"] and h.hexdigest() == sweep["digests"][name]["sha256"]


def test_gpu_test_shapes_reach_every_entry_of_every_launch_table(golden, plan):
    """A wrong table entry launches a kernel whose tile count does not match its LDS plan, and only a launch shows it: the shape lists
    of the GPU stage tests (stage_shapes.py) must between them run every instantiation."""
    fam = golden["families"]
    reached = set()
    for (B, H, W) in stage_shapes.RESSTAGE16:
        reached.add(tuple(plan(RESSTAGE16, 16, B, H, W)[:6]))
    for (B, H, W) in stage_shapes.RESSTAGE32:
        reached.add(tuple(plan(RESSTAGE32, 32, B, H, W)[:6]))
    for (cin, B, H, W) in stage_shapes.CONVPOOL32:
        reached.add(tuple(plan(CONVPOOL32, cin, B, H, W)[:6]))
    for S, batches in stage_shapes.STAGE32_PM_BATCHES.items():
        for B in batches:
            for force in (1, 0):
                reached.add(tuple(plan(RESSTAGE32, 32, B, S, S, pm_force=force)[:6]))
    assert all(r[0] == 0 for r in reached)
    reached = {(fam[r[1]],) + r[2:] for r in reached}
    assert len(TABLES) == 51 and len(set(TABLES)) == 51
    assert reached == set(TABLES), "never launched: %r; not in a table: %r" % (sorted(set(TABLES) - reached), sorted(reached - set(TABLES)))



def test_row_limit_cases_reach_every_kernel_family_and_instantiation(golden):
    """test_gpu_stage_rows.py pins the device row limit, the write bounds and the isolation of leaves per launch; every instantiation
    handles the last, partly filled group of leaves in its own code, so its cases (stage_shapes.row_limit_cases) must reach every entry of
    every launch table and the two families behind their own plan exports (k_resstage16_pp, k_convpool32_pm) -- each through the export
    that has its entry point's per-call knob."""
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB)
    i32, i64, out_t = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.rp_debug_stage_plan.argtypes = [i32, i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_convpool_plan.argtypes = [i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_stage16_plan.argtypes = [i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    n_cu, lds = golden["devices"][0]["n_cu"], golden["devices"][0]["lds_per_cu"]
    fam = golden["families"] + ["k_convpool32_pm", "k_resstage16_pp"]  # appended behind the recorded families (FAM_CP_PM, FAM_RS16_PP)
    cases = stage_shapes.row_limit_cases()
    assert len(cases) == len(set(cases))
    reached = set()
    for (entry, cin, B, H, W, knob) in cases:
        out = (ctypes.c_int64 * 10)()
        if entry == stage_shapes.ENTRY_RESSTAGE16:
            rc = L.rp_debug_stage16_plan(B, H, W, n_cu, lds, 2, 1, knob, out)
        elif entry == stage_shapes.ENTRY_CONVPOOL32:
            rc = L.rp_debug_convpool_plan(cin, B, H, W, n_cu, lds, 2, 1, knob, out)
        else:
            rc = L.rp_debug_stage_plan(entry, cin, B, H, W, n_cu, lds, 2, 1, knob, out)
        assert rc == 0 and out[5] >= 1, (entry, cin, B, H, W, knob)
        reached.add((fam[out[0]],) + tuple(out[1:5]))
    want = set(TABLES) | {("k_convpool32_pm", 25, 4, 32, 0), ("k_resstage16_pp", 50, 4, 16, 0)}
    assert len(want) == 53
    assert reached == want, "never launched: %r; not in a table: %r" % (sorted(want - reached), sorted(reached - want))
