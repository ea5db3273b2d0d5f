"""CPU-only checks of the lag window (muse_batch_set_lag_window): the numpy statement of its definition (tests/_window.py) is pinned
to the reference -- with L >= n / 2 it reproduces the oracle's own (lag, mv), on random rows and on the reference's known-answer
table -- the two functions and MUSE_LAG_WINDOW_MAX exist on every layer, nothing crashes without a GPU, and the three host mirrors
carry Batch.RunWindowed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _window as W
from _load import ROOT, pkg

EXPORTS = ("muse_batch_set_lag_window", "muse_batch_lag_window")


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


@pytest.mark.parametrize("N", [2, 3, 8, 100, 255, 480, 512, 1433])
def test_helper_reproduces_the_oracle_for_a_full_window(oracle, N):
    rng = np.random.default_rng(N)
    ref, rows = W.make_case(N, 60, seed=N)
    rows = np.concatenate([rows, rng.standard_normal((40, N))])
    X, n = oracle.ref_spectrum(ref)
    for y in rows:
        cc, lag, mv, _ = oracle.xcorr_with_x(X, y, n)
        for L in (n // 2, n // 2 + 1, n, 10 * n):
            for fn in (W.windowed, W.windowed_fast):
                l, v, _ = fn(cc, n, L)
                assert l == lag and (v == mv or (np.isnan(v) and np.isnan(mv))), (N, L, fn.__name__)
        # and the slow and the vectorised statement agree for every window
        for L in (0, 1, 7, 8, 15, 16, 31, 63):
            a, b = W.windowed(cc, n, L), W.windowed_fast(cc, n, L)
            assert a[0] == b[0] and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1]))) and a[2] == b[2]
            assert abs(a[0]) <= min(L, n // 2)


def test_helper_on_the_golden_xcorr_with_x_cases(golden, oracle):   # xcorr_test.go:204-286, padded to n = 8
    n = 8
    for c in golden["xcorr_with_x"]["cases"]:
        X, _ = oracle.ref_spectrum(c["x"], n)
        cc, lag, mv, _ = oracle.xcorr_with_x(X, c["y"], n)
        for fn in (W.windowed, W.windowed_fast):
            assert fn(cc, n, n // 2)[:2] == (lag, mv)
            assert fn(cc, n, 63)[:2] == (lag, mv)
        if cc is None:                                               # the constant series: (nil, 0, 0) for every window
            assert W.windowed(cc, n, 0) == (0, 0.0, False)
            continue
        assert lag == c["idx"] and np.sign(mv) == c["sign"]          # (the table's answer: the helper is pinned to the reference)
        # a window that leaves the winner out finds the best of what is left, first index first
        for L in range(0, n // 2 + 1):
            l, v, _ = W.windowed(cc, n, L)
            idx = W.window_indices(n, L)
            assert abs(l) <= L and abs(v) == np.max(np.abs(cc[idx]))
            first = idx[np.nonzero(np.abs(cc[idx]) == abs(v))[0][0]]
            assert l == (first if first <= n // 2 else first - n)


def test_window_definition_edge_cases():
    n = 16
    cc = np.zeros(n)
    assert W.windowed(cc, n, 3) == (0, 0.0, False)                   # only zeros: index 0 stands
    cc[:] = np.nan
    l, v, _ = W.windowed(cc, n, 3)
    assert l == 0 and np.isnan(v)                                    # only NaN: lag 0 and cc[0]
    cc = np.zeros(n)
    cc[2] = cc[14] = -0.5                                            # lag 2 and lag -2 tie: the first index (lag 2) wins
    assert W.windowed(cc, n, 3)[:2] == (2, -0.5) and W.windowed(cc, n, 3)[2]
    cc[9] = 0.9                                                      # index 9 = lag -7: outside +-3, inside +-7
    assert W.windowed(cc, n, 3)[:2] == (2, -0.5) and W.windowed(cc, n, 7)[:2] == (-7, 0.9)
    cc[8] = 1.0                                                      # index n / 2 is lag +n/2
    assert W.windowed(cc, n, 8)[:2] == (8, 1.0) and W.windowed(cc, n, 7)[:2] == (-7, 0.9)


def test_exports_declared_exported_and_bound(muse):
    hdr = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    m = re.search(r"#define\s+MUSE_LAG_WINDOW_MAX\s+(\d+)", hdr)
    assert m, "muse_hip.h does not define MUSE_LAG_WINDOW_MAX"
    assert int(m.group(1)) == muse.binding.MUSE_LAG_WINDOW_MAX >= 15
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), "muse_hip.h does not declare %s" % name
        assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
        assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    assert muse.binding.load().muse_abi_version() == 5               # backward compatible additions: the ABI version stays


def test_no_gpu_fails_loudly_not_with_a_crash(muse):
    """Without a device no context, hence no batch, can exist: the engine a windowed score needs fails with MUSE_ERR_NO_DEVICE,
    and the two functions answer a NULL handle with MUSE_ERR_INVALID instead of touching it."""
    import torch
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    assert L.muse_batch_set_lag_window(None, 15) == B.MUSE_ERR_INVALID
    assert L.muse_batch_lag_window(None, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_batch_score(None) == B.MUSE_ERR_INVALID
    if torch.cuda.is_available():
        return
    with pytest.raises(muse.MuseError) as e:
        eng = muse.Engine(0)
        dg = muse.DeviceGroup.from_rows(eng, np.zeros((2, 8)))
        db = muse.DeviceBatch(eng, dg, np.arange(8.0))
        db.set_lag_window(3)
        db.score()
    assert e.value.status == B.MUSE_ERR_NO_DEVICE


def test_run_windowed_exists_in_the_three_mirrors(muse):
    assert callable(getattr(muse.Batch, "RunWindowed", None))
    assert callable(getattr(muse.DeviceBatch, "set_lag_window", None)) and callable(getattr(muse.DeviceBatch, "lag_window", None))
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bvoid\s+RunWindowed\s*\(", hpp) and "muse_batch_set_lag_window" in hpp
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func \(b \*Batch\) RunWindowed\(groupByLabels \[\]string\) error", go) and "C.muse_batch_set_lag_window(" in go
    # the C++ program the GPU suite runs is built with the rest
    assert os.path.exists(muse.build.build_window_test())
