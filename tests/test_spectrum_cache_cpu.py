"""The spectrum cache's policy (capi_batch.hip, spectrum_cache_policy) is a pure host function: which groups
are cached, how many bytes that takes, and when it is declined.  Reached through muse_test_spectrum_cache_policy -- no GPU."""
import ctypes

import pytest

from _load import pkg

NONE, BUILD, DECLINED = 0, 1, 2
PAIR_BYTES = 65536 + 128


@pytest.fixture(scope="module")
def policy():
    m = pkg()
    m.build.build()
    lib = m.binding.load()

    def f(rows, N=4096, f32=0, mode=1, min_rows=-1, free_bytes=1 << 60, budget=-1):
        d, r, b = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
        m.binding.check(lib.muse_test_spectrum_cache_policy(rows, N, f32, mode, min_rows, free_bytes, budget,
                                                           ctypes.byref(d), ctypes.byref(r), ctypes.byref(b)))
        return int(d.value), int(r.value), int(b.value)
    return f


def test_smallest_cached_group(policy):
    assert policy(65535) == (NONE, 0, 0)
    assert policy(65536) == (BUILD, 65536, 32768 * PAIR_BYTES)
    assert policy(1000000) == (BUILD, 1000000, 500000 * PAIR_BYTES)


def test_half_of_the_free_memory(policy):
    B = 32768 * PAIR_BYTES
    assert policy(65536, free_bytes=2 * B) == (BUILD, 65536, B)
    assert policy(65536, free_bytes=2 * B - 1) == (DECLINED, 65536, B)
    assert policy(65536, free_bytes=0) == (DECLINED, 65536, B)


def test_budget_override(policy):
    B = 32768 * PAIR_BYTES
    assert policy(65536, free_bytes=0, budget=B)[0] == BUILD          # the override replaces the free-memory rule
    assert policy(65536, free_bytes=1 << 60, budget=B - 1)[0] == DECLINED
    assert policy(65536, free_bytes=1 << 60, budget=0)[0] == DECLINED  # 0 = always decline


def test_what_is_never_cached(policy):
    assert policy(1 << 20, f32=1)[0] == NONE       # a float64 spectrum is 4 x a float32 group's rows
    assert policy(1 << 20, N=2048)[0] == NONE      # FFT length 2048
    assert policy(1 << 20, N=5000)[0] == NONE      # FFT length 8192
    assert policy(1 << 20, mode=0)[0] == NONE
    assert policy(1 << 20, N=2049)[0] == BUILD     # FFT length 4096 with a leading zero pad
    assert policy(1 << 20, N=3000)[0] == BUILD


def test_an_odd_group_caches_all_but_its_last_row(policy):
    assert policy(65537) == (BUILD, 65536, 32768 * PAIR_BYTES)
    assert policy(1001, min_rows=2) == (BUILD, 1000, 500 * PAIR_BYTES)
    assert policy(3, min_rows=0) == (BUILD, 2, PAIR_BYTES)
    assert policy(1, min_rows=0) == (NONE, 0, 0)   # no pair of two rows
