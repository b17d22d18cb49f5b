"""Host-side checks of the position-major stage kernels: which kernel rp_nn_resstage32 picks per launch shape, and that the
LDS swizzle keeps every lane group of a 16-byte read / write on different banks.  No GPU needed: the two helpers are plain host code."""
import ctypes
import os

import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "resource_packing_self_play_amd", "csrc", "librp_engine.so")


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (its HIP runtime first: a later _lib.load() in this process refuses two of them)
    L = ctypes.CDLL(LIB)
    L.rp_debug_stage32_pm_pick.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    L.rp_debug_stage32_pm_swz.argtypes = [ctypes.c_int32]
    return L


def test_dispatch_picks_position_major_for_the_flagship_and_not_for_small_batches(lib):
    pick = lib.rp_debug_stage32_pm_pick
    for S in (3, 5):
        assert pick(30000, S, S) == 1 and pick(32768, S, S) == 1   # c3: ~30 000 leaves of 32 768 slots
        assert pick(64, S, S) == 0 and pick(4096, S, S) == 0       # c2: 256 tasks of sixteen leaves
        assert pick(0, S, S) == 0
    assert pick(30000, 4, 4) == 0 and pick(30000, 3, 5) == 0 and pick(30000, 13, 13) == 0  # other shapes keep k_resstage32


def test_swizzle_is_free_of_bank_conflicts(lib):
    swz = [lib.rp_debug_stage32_pm_swz(n) for n in range(16)]
    assert all(0 <= s < 8 for s in swz)
    # ds_read_b128: four groups of sixteen lanes, 64 banks of 4 bytes = sixteen 16-byte units; lane (leaf n, group g) reads quad 2 g + h
    a = list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))
    b = list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))
    for group in (a, b, [l + 32 for l in a], [l + 32 for l in b]):
        for h in (0, 1):
            units = {((l & 15) * 8 + ((2 * (l >> 4) + h) ^ swz[l & 15])) % 16 for l in group}
            assert len(units) == 16
    # ds_write_b128: eight groups of eight consecutive lanes, 32 banks = eight units; lane (n, g) writes quads g and 4 + g
    for first in range(0, 64, 8):
        for mt in (0, 1):
            units = {((4 * mt + (l >> 4)) ^ swz[l & 15]) % 8 for l in range(first, first + 8)}
            assert len(units) == 8
