"""Host-side checks of the position-paired 16-channel 10x10 stage kernel (k_resstage16_pp): which kernel plan_resstage16
picks, the launch shape, the wave roles' (tile, tap) tables and the LDS swizzle.  rp_debug_stage_plan keeps the RP_STAGE16_PP knob at 0
(its recorded plans are k_resstage16's); rp_debug_stage16_plan exposes it (0: old kernel, 1: new kernel, -1: the cost rule).  The
addresses come from the functions the kernel forms its per-lane bases and immediates with.  No GPU needed."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "resource_packing_self_play_amd", "csrc", "librp_engine.so")
N_CU, LDS_PER_CU = 256, 160 * 1024
FAM_RS16, FAM_RS16_PP = 1, 9  # FAM_RS16_PP is appended behind the families recorded in tests/golden/stage_plans.json
LDS_BYTES = (64 + 102 * 8 * 16) * 4  # [4][16] biases, [guard + 100 positions + guard][8 leaves][16 floats]
# rc, family, nt (tiles), waves, cin, tail, imgw, wave_floats, lds -- then grid, block
PP_PLAN = [0, FAM_RS16_PP, 50, 4, 16, 0, 8, 0, LDS_BYTES]
# lane groups that a 16-byte LDS read / write is served in, one LDS cycle each: sixteen 16-byte units per read cycle, eight per write cycle
READ_GROUPS = [[l + h for l in g] for h in (0, 32) for g in (list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                                                             list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)))]
WRITE_GROUPS = [list(range(f, f + 8)) for f in range(0, 64, 8)]


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    i32, i64, out_t = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
    L.rp_debug_stage_plan.argtypes = [i32, i32, i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_stage16_plan.argtypes = [i64, i32, i32, i32, i64, i32, i32, i32, out_t]
    L.rp_debug_stage16_pp_off.argtypes = [i32, i32, i32]
    L.rp_debug_stage16_pp_role.argtypes = [i32, ctypes.POINTER(i32)]
    L.rp_debug_stage16_pp_lane_off.argtypes = [i32, i32, i32]
    return L


@pytest.fixture(scope="module")
def plans(lib):
    def new(B, H, W, pp, n_cu=N_CU, lds=LDS_PER_CU, wgs=2, tail=1):
        out = (ctypes.c_int64 * 10)()
        rc = lib.rp_debug_stage16_plan(B, H, W, n_cu, lds, wgs, tail, pp, out)
        return [rc] + list(out)

    def old(B, H, W, n_cu=N_CU, lds=LDS_PER_CU, wgs=2, tail=1):
        out = (ctypes.c_int64 * 10)()
        rc = lib.rp_debug_stage_plan(0, 16, B, H, W, n_cu, lds, wgs, tail, -1, out)
        return [rc] + list(out)
    return new, old


@pytest.fixture(scope="module")
def roles(lib):
    """per role: tiles [(position of member A, of member B)], entries [(tap, tile index, zeroed A, zeroed B)] in execution order"""
    res = []
    for role in range(4):
        buf = (ctypes.c_int32 * (2 + 2 * 13 + 4 * 100))()
        n = lib.rp_debug_stage16_pp_role(role, buf)
        np_, ne = buf[0], buf[1]
        assert n == 2 + 2 * np_ + 4 * ne
        tiles = [(buf[2 + 2 * k], buf[3 + 2 * k]) for k in range(np_)]
        o = 2 + 2 * np_
        res.append((tiles, [tuple(buf[o + 4 * e:o + 4 * e + 4]) for e in range(ne)]))
    return res


def _taps(p):
    """the taps of output position p whose input pixel lies inside the 10x10 image"""
    return {t for t in range(9) if 0 <= p // 10 + t // 3 - 1 < 10 and 0 <= p % 10 + t % 3 - 1 < 10}


@pytest.mark.parametrize("B", (30000, 32768))
def test_cost_rule_picks_the_new_kernel_for_the_flagship_batches(plans, B):
    new, old = plans
    got = new(B, 10, 10, -1)
    assert got[:9] == PP_PLAN and got[10] == 256
    assert got[9] == min((B + 7) // 8, 2 * N_CU) == 512
    assert old(B, 10, 10)[1] == FAM_RS16  # the recorded entry stays on k_resstage16


@pytest.mark.parametrize("B", (4096, 1030, 64, 1))
def test_cost_rule_keeps_the_old_kernel_for_small_batches(plans, B):
    new, old = plans
    got = new(B, 10, 10, -1)
    assert got[0] == 0 and got[1] == FAM_RS16 and got == old(B, 10, 10)
    assert got[2:6] == [6, 4, 16, 1]  # k_resstage16<6, true>


def test_cost_rule_figures_checked_by_hand(plans):
    """In quarter tile-taps: pm_rounds_cost(B, 8, 512) * 396 against pm_rounds_cost(B, 1, 2048) * (4 * 6 * 9 + 9), rounds(B) + 3 *
    rounds(0.92 B), and only where the typical wave gives a workgroup more than one task (0.92 B / 8 > 512).  30 000 rows: 29 * 396 =
    11 484 < 57 * 225 = 12 825; 32 768: 32 * 396 < 61 * 225; 6 680 rows are the first to pick it (8 * 396 < 16 * 225), 8 906 the first to drop
    it again (12 * 396 > 20 * 225: a third round of tasks for the typical wave), and from 14 337 rows on it stays."""
    new, _ = plans

    def cost(B, k, units):
        r = lambda rows: -(-(-(-rows // k)) // units)
        return r(B) + 3 * r(max(1, int(0.92 * B)))
    assert cost(30000, 8, 512) * 396 == 11484 and cost(30000, 1, 2048) * 225 == 12825
    assert cost(32768, 8, 512) == 32 and cost(32768, 1, 2048) == 61
    for B in list(range(1, 6000, 7)) + [4096, 6679, 6680, 8905, 8906, 14336, 14337, 30000, 32768, 100000]:
        want = -(-max(1, int(0.92 * B)) // 8) > 512 and cost(B, 8, 512) * 396 < cost(B, 1, 2048) * 225
        assert (new(B, 10, 10, -1)[1] == FAM_RS16_PP) == want, B
    assert new(6679, 10, 10, -1)[1] == FAM_RS16 and new(6680, 10, 10, -1)[1] == FAM_RS16_PP and new(8906, 10, 10, -1)[1] == FAM_RS16
    assert all(new(B, 10, 10, -1)[1] == FAM_RS16_PP for B in range(14337, 40000, 13))


def test_a_device_with_64_kb_of_lds_never_picks_it(plans):
    new, old = plans
    for B in (1, 64, 4096, 30000, 32768, 1000000):
        got = new(B, 10, 10, -1, lds=64 * 1024)
        assert got[1] == FAM_RS16 and got == old(B, 10, 10, lds=64 * 1024)  # two workgroups per CU do not fit
    assert new(30000, 10, 10, -1, lds=2 * LDS_BYTES)[1] == FAM_RS16_PP and new(30000, 10, 10, -1, lds=2 * LDS_BYTES - 1)[1] == FAM_RS16
    assert new(30000, 10, 10, 1, lds=LDS_BYTES - 1)[1] == FAM_RS16  # not even when forced: the image does not fit


@pytest.mark.parametrize("B", (1, 7, 8, 9, 23, 4096, 4099, 30000))
def test_the_knob_is_obeyed(plans, B):
    new, old = plans
    got = new(B, 10, 10, 1)
    assert got[:9] == PP_PLAN and got[9] == min((B + 7) // 8, 2 * N_CU) and got[10] == 256
    assert new(B, 10, 10, 1, n_cu=8)[9] == min((B + 7) // 8, 16) and new(B, 10, 10, 1, wgs=1)[9] == min((B + 7) // 8, N_CU)
    assert new(B, 10, 10, 1, lds=64 * 1024)[9] == min((B + 7) // 8, N_CU)  # one workgroup per CU fits
    off = new(B, 10, 10, 0)
    assert off[1] == FAM_RS16 and off == old(B, 10, 10)


def test_other_shapes_keep_their_kernels(plans):
    new, old = plans
    rng = random.Random(16)
    shapes = [(10, 9), (9, 10), (5, 5), (10, 11), (20, 5), (25, 25), (1, 1), (11, 11)]
    for H, W in shapes:
        for pp in (-1, 0, 1):
            B = rng.choice((1, 64, 4096, 30000))
            assert new(B, H, W, pp) == old(B, H, W), (B, H, W, pp)
    assert new(0, 10, 10, 1) == old(0, 10, 10) and new(-1, 10, 10, 1)[0] != 0


def test_every_position_belongs_to_one_tile_and_every_role_issues_99_tile_taps(roles):
    seen = []
    for tiles, entries in roles:
        seen += [p for t in tiles for p in t]
        assert len(entries) == 99
        assert [e[0] for e in entries] == sorted(e[0] for e in entries)  # tap-major: every output sums its taps in rising order
        for k, (pa, pb) in enumerate(tiles):
            assert {e[0] for e in entries if e[1] == k} == _taps(pa) | _taps(pb)
            assert len([e for e in entries if e[1] == k]) == len(_taps(pa) | _taps(pb))
            for tap, _, za, zb in (e for e in entries if e[1] == k):
                assert za == (tap not in _taps(pa)) and zb == (tap not in _taps(pb))  # a member without the tap multiplies zeros
        assert all(a[1] != b[1] for a, b in zip(entries[0::2], entries[1::2]))  # the kernel runs two entries at a time, as two chains
    assert sorted(seen) == list(range(100))
    assert [len(t) for t, _ in roles] == [12, 12, 13, 13]
    by_taps = sorted(len(_taps(pa) | _taps(pb)) for t, _ in roles for pa, pb in t)
    assert by_taps == [6] * 18 + [9] * 32
    # only the two corner pairs take a tap that one member lacks
    mixed = {t[e[1]] for t, es in roles for e in es if e[2] or e[3]}
    assert mixed == {(0, 9), (90, 99)}


def test_lane_addresses_are_the_stored_places_and_free_of_bank_conflicts(lib, roles):
    off, lane_off = lib.rp_debug_stage16_pp_off, lib.rp_debug_stage16_pp_lane_off
    image = range(8 * 64, 101 * 8 * 64)  # bytes from the front guard
    places = {off(p, l, q) for p in range(100) for l in range(8) for q in range(4)}
    assert len(places) == 3200 and all(a % 16 == 0 and a in image for a in places)
    for role, (tiles, entries) in enumerate(roles):
        for e, (tap, k, za, zb) in enumerate(entries):
            addr = [lane_off(role, e, lane) for lane in range(64)]
            assert all(0 <= a <= LDS_BYTES - 256 - 16 for a in addr)
            for lane in range(64):
                n, g = lane & 15, lane >> 4
                if (zb if n >> 3 else za):
                    continue  # zeroed operand: anywhere inside the buffer
                q = tiles[k][n >> 3] + (tap // 3 - 1) * 10 + tap % 3 - 1
                assert addr[lane] == off(q, n & 7, g), (role, e, lane)
            for group in READ_GROUPS:
                assert len({(addr[l] // 16) % 16 for l in group}) == 16, (role, e)
        for k, (pa, pb) in enumerate(tiles):
            addr = [lane_off(role, -1 - k, lane) for lane in range(64)]
            assert all(addr[lane] == off((pa, pb)[(lane & 15) >> 3], lane & 7, lane >> 4) for lane in range(64))
            for group in WRITE_GROUPS:
                assert len({(addr[l] // 16) % 8 for l in group}) == 8, (role, k)
