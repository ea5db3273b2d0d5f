"""CPU-only checks of the windowed Muse.Run (muse_batch_run_rows_windowed / _run_row_ptrs_windowed / _run_group_rows_windowed): the
three exports exist on every layer with their argument counts, the host mirrors carry Muse.RunWindowed, NULL handles are answered
with an argument error and without a crash, and the planner of the split-K kernels (muse_test_window_rows_plan, a pure host function)
keeps its promises: 1 <= S <= chunks, slices that cover every chunk exactly once, no split of short series or of groups that
already fill the chip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _load import ROOT, pkg

EXPORTS = {"muse_batch_run_rows_windowed": 8, "muse_batch_run_row_ptrs_windowed": 7, "muse_batch_run_group_rows_windowed": 8}
HOOKS = {"muse_test_window_rows_plan": 5, "muse_test_window_rows_slices": 2, "muse_test_run_rows_windowed_scores": 7}
WIN_KC = 1024            # samples per chunk (xcorr_kernels.h)
FULL_SPLIT = 16          # up to this many slices a slice may be one chunk (WIN_ROWS_FULL_SPLIT) ...
MIN_CHUNKS = 2           # ... beyond, at least this many chunks per slice (WIN_ROWS_MIN_CHUNKS): both measured, DESIGN 4.9


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(muse_[a-z0-9_]+)\s*\(([^)]*)\)", hdr):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_exports_declared_exported_and_bound(muse):
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for header, names in (("muse_hip.h", EXPORTS), ("muse_hip_test.h", HOOKS)):
        declared = _declared(header)
        for name, nargs in names.items():
            assert declared.get(name) == nargs, "%s: %s declared with %s arguments" % (header, name, declared.get(name))
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert len(muse.binding.SIGNATURES[name][1]) == nargs, "binding.SIGNATURES: %s" % name
    # exactly these three: nothing else of the kind
    assert {n for n in exported if re.search(r"_(rows|row_ptrs)_windowed$", n)} == set(EXPORTS)
    # the hooks are outside the drop-in boundary
    assert not any(h in _declared("muse_hip.h") for h in HOOKS)


def test_mirrors_name_the_exports_and_run_windowed(muse):
    src = lambda *p: open(os.path.join(ROOT, "go-muse_amd", *p)).read()
    py, hpp, go = src("muse.py"), src("host", "muse.hpp"), src("go", "muse_hip.go")
    for name in EXPORTS:
        assert name in py, name
    for meth in ("run_rows_windowed", "run_row_ptrs_windowed", "run_group_rows_windowed"):
        assert callable(getattr(muse.DeviceBatch, meth))
    assert callable(muse.Muse.RunWindowed)
    # C++: pointers per row and resident rows; Go: the packed form (cgo may not pass an array of Go pointers)
    assert "muse_batch_run_row_ptrs_windowed(" in hpp and "muse_batch_run_group_rows_windowed(" in hpp
    muse_cls = hpp[hpp.index("class Muse {"):]
    assert re.search(r"void RunWindowed\(const std::vector<SeriesPtr> &compGraphs\)", muse_cls)
    assert "C.muse_batch_run_rows_windowed(" in go
    assert re.search(r"func \(m \*Muse\) RunWindowed\(compGraphs \[\]\*Series\) error", go)
    prog = src("host", "muse_rows_window_test.cpp")
    assert "RunWindowed" in prog and os.path.exists(muse.build.build_rows_window_test())


def test_python_run_windowed_refuses_a_window_outside_the_cap(muse):
    """Muse.RunWindowed checks Results.MaxLag before anything touches a device -- but a Muse needs a device to exist, so the
    check is exercised on an object built without its constructor"""
    m = object.__new__(muse.Muse)
    m.refN = 8
    for bad in (-1, muse.binding.MUSE_LAG_WINDOW_MAX + 1):
        m.Results = muse.NewResults(bad, 5, 0.0, muse.SignFilter_ANY)
        with pytest.raises(muse.MuseError) as e:
            m.RunWindowed([muse.NewSeries(np.arange(8.0), None)])
        assert e.value.status == muse.binding.MUSE_ERR_UNSUPPORTED
    assert m.RunWindowed([]) is None            # muse.go:47-50: nothing to compare


def _slices(chunks, S):
    return [(s * chunks // S, (s + 1) * chunks // S) for s in range(S)]


@pytest.mark.parametrize("num_cus", [1, 64, 256])
@pytest.mark.parametrize("N", [2, 480, 1024, 1025, 4096, 40000, 65536])
def test_planner_properties(muse, N, num_cus):
    chunks = (N + WIN_KC - 1) // WIN_KC
    # the longest length at one block on a very wide part shows the planner's constants (1: the planner is switched off)
    S_wide, _ = muse.window_rows_plan(1, 65536, 1 << 20)
    assert S_wide in (1, 64 // MIN_CHUNKS)
    min_cps = 1 if S_wide > 1 else 64                         # the smallest slice the planner may ever make
    seen_split = False
    for M in range(1, 5001):
        S, cps = muse.window_rows_plan(M, N, num_cus)
        blocks = (M + 15) // 16
        assert 1 <= S <= chunks, (M, N, num_cus, S)
        sl = _slices(chunks, S)
        assert sl[0][0] == 0 and sl[-1][1] == chunks and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))   # every chunk exactly once
        assert all(hi > lo for lo, hi in sl) and max(hi - lo for lo, hi in sl) == cps
        if chunks < 2 * min_cps or blocks >= num_cus:
            assert S == 1, (M, N, num_cus, S)
        if S > 1:
            seen_split = True
            assert min(hi - lo for lo, hi in sl) >= (MIN_CHUNKS if S > FULL_SPLIT else 1)
            assert blocks * S <= num_cus                     # never more workgroups than CUs
    if S_wide == 1:                                          # the planner is switched off: it says 1 everywhere
        assert not seen_split


def test_null_handles_are_argument_errors_and_no_engine_exists_without_a_device(muse):
    """every new entry point answers NULL handles with MUSE_ERR_INVALID and nothing crashes; without a device no engine, hence no
    template, can be made (MUSE_ERR_NO_DEVICE at muse_ctx_create), so the exports' own device check is out of a test's reach"""
    import torch
    B = muse.binding
    L = B.load()
    INV = B.MUSE_ERR_INVALID
    rec = np.zeros(1, dtype=B.RECORD_DTYPE)
    st = ctypes.c_uint8(7)
    x = np.zeros((2, 16))
    # NULL template / outputs: argument errors, with or without a device
    assert L.muse_batch_run_rows_windowed(None, B.dptr(x), 2, 16, 7, 0, B.recptr(rec), ctypes.byref(st)) == INV
    assert L.muse_batch_run_row_ptrs_windowed(None, None, 2, 7, 0, B.recptr(rec), ctypes.byref(st)) == INV
    assert L.muse_batch_run_group_rows_windowed(None, None, None, 2, 7, 0, B.recptr(rec), ctypes.byref(st)) == INV
    lag, mv = np.zeros(2, dtype=np.int32), np.zeros(2)
    assert L.muse_test_run_rows_windowed_scores(None, B.dptr(x), 2, 16, 7, B.i32ptr(lag), B.dptr(mv)) == INV
    assert L.muse_test_window_rows_slices(None, 2) == INV
    S = ctypes.c_int32(0)
    assert L.muse_test_window_rows_plan(0, 4096, 256, ctypes.byref(S), None) == INV
    assert L.muse_test_window_rows_plan(5, 1, 256, ctypes.byref(S), None) == INV
    assert L.muse_test_window_rows_plan(5, 4096, 0, ctypes.byref(S), None) == INV
    assert L.muse_test_window_rows_plan(5, 4096, 256, None, None) == INV
    assert L.muse_test_window_rows_plan(5, 4096, 256, ctypes.byref(S), None) == 0 and S.value >= 1
    if not torch.cuda.is_available():
        with pytest.raises(muse.MuseError) as e:          # no engine, hence no template: the way in is closed loudly
            muse.Engine(0)
        assert e.value.status == B.MUSE_ERR_NO_DEVICE
