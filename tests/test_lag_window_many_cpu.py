"""CPU-only checks of the windowed many-references pass (muse_batch_score_many_windowed / _run_many_windowed): the two exports
exist on every layer, bad lists are answered without a device and without a crash, the three host mirrors carry RunManyWindowed,
and the planner (muse_test_window_many_plan, a pure host function) cuts any R references into consecutive, greedy launches of at
most 128 packed rows whose staged images do not collide on the LDS banks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _load import ROOT, pkg

EXPORTS = ("muse_batch_score_many_windowed", "muse_batch_run_many_windowed")
PLAN_LS = (0, 1, 3, 7, 8, 15, 16, 31, 32, 63)
PACK_MAX_ROWS = 48       # a window of more rows fills four tiles by itself and is not packed (WINM_PACK_MAX_ROWS)
IMG_BUDGET = 4608        # doubles of staged reference images per launch (xcorr_kernels.h, WINM_IMG_DOUBLES)


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def test_exports_declared_exported_and_bound(muse):
    hdr = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, hdr), "muse_hip.h does not declare %s" % name
        assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
        assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    test_hdr = open(os.path.join(ROOT, "include", "muse_hip_test.h")).read()
    assert re.search(r"\bmuse_test_window_many_plan\s*\(", test_hdr) and "muse_test_window_many_plan" in exported
    assert "muse_test_window_many_plan" in muse.binding.SIGNATURES
    assert muse.binding.load().muse_abi_version() == 5               # additions: the ABI version stays


def test_bad_lists_are_invalid_without_a_device(muse):
    B = muse.binding
    L = B.load()
    INV = B.MUSE_ERR_INVALID
    one = (ctypes.c_void_p * 1)(None)
    two = (ctypes.c_void_p * 2)(None, None)
    assert L.muse_batch_score_many_windowed(None, 2, 7) == INV                   # NULL list
    assert L.muse_batch_score_many_windowed(two, 0, 7) == INV                    # R < 1
    assert L.muse_batch_score_many_windowed(two, -3, 7) == INV
    assert L.muse_batch_score_many_windowed(one, 1, 7) == INV                    # NULL entry
    assert L.muse_batch_score_many_windowed(two, 2, 7) == INV
    assert L.muse_batch_score_many_windowed(two, 2, -1) == INV                   # negative window (the NULL entry comes first either way)
    assert L.muse_batch_score_many_windowed(None, 1, -1) == INV
    run = lambda arr, R, lag: L.muse_batch_run_many_windowed(arr, R, None, 0, lag, 5, 0.0, 0, 1, None, None, None, None, None)
    assert run(None, 2, 7) == INV and run(two, 0, 7) == INV and run(one, 1, 7) == INV and run(two, 2, -1) == INV
    with pytest.raises(ValueError):
        muse.score_many_windowed([], 7)
    # the hook itself refuses what the planner is not made for
    n = ctypes.c_int32(0)
    assert L.muse_test_window_many_plan(0, 7, ctypes.byref(n), None, None, None, None, None) == INV
    assert L.muse_test_window_many_plan(4, -1, ctypes.byref(n), None, None, None, None, None) == INV
    assert L.muse_test_window_many_plan(4, B.MUSE_LAG_WINDOW_MAX + 1, ctypes.byref(n), None, None, None, None, None) == INV
    assert L.muse_test_window_many_plan(4, 7, None, None, None, None, None, None) == INV


def test_run_many_windowed_exists_in_the_three_mirrors(muse):
    for name in ("RunManyWindowed", "run_many_windowed", "score_many_windowed", "scores_many_windowed"):
        assert callable(getattr(muse, name, None)), name
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bstatic\s+void\s+RunManyWindowed\s*\(", hpp) and "muse_batch_run_many_windowed(" in hpp
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func RunManyWindowed\(batches \[\]\*Batch, groupByLabels \[\]string\) error", go)
    assert "C.muse_batch_run_many_windowed(" in go


def _fits(refs, L):
    """`refs` references of window L in one launch: 128 packed rows, and their images at the shortest chunk inside the budget"""
    W = 2 * L + 1
    if W > PACK_MAX_ROWS:                                  # (four tiles per reference: measured no faster packed -- one launch each)
        return refs == 1
    img = 256 + 2 * L
    while img % 32 != (W + 2) % 32:
        img += 1
    return refs * W <= 128 and refs * img <= IMG_BUDGET


@pytest.mark.parametrize("L", PLAN_LS)
def test_planner(muse, L):
    W = 2 * L + 1
    for R in range(1, 41):
        p = muse.window_many_plan(R, L)
        of, tiles, k = p["launch_of"], p["tiles_of"], p["launches"]
        assert len(of) == R and len(tiles) == k and 1 <= k <= R
        # every reference in exactly one launch; launches consecutive and in order
        assert of[0] == 0 and of[-1] == k - 1 and np.all((np.diff(of) == 0) | (np.diff(of) == 1))
        counts = np.bincount(of, minlength=k)
        assert counts.sum() == R and np.all(counts >= 1)
        rows = counts * W
        assert np.all(rows <= 128)
        assert np.array_equal(tiles, (rows + 15) // 16) and np.all(tiles <= 8) and np.all(tiles >= 1)
        assert int(tiles.sum()) <= R * ((W + 15) // 16)                          # packing never costs tiles
        # greedy: no launch but the last could have taken the next reference
        for l in range(k - 1):
            assert _fits(int(counts[l]), L) and not _fits(int(counts[l]) + 1, L), (R, L, l, counts)
        assert _fits(int(counts[-1]), L) or counts[-1] == 1
        assert p["max_refs"] == max(c for c in range(1, 129) if _fits(c, L) or c == 1)
        if W > PACK_MAX_ROWS:
            assert k == R and np.all(counts == 1)                                # a reference that fills its tiles: R single passes
        # the chunk stays a multiple of 256 samples that divides the single-reference kernel's 1024 (piece p -> wave p mod 4,
        # and the tables' zero padding to whole chunks of 1024 covers every chunk), and the images fit the budget
        for l in range(k):
            kc, img = int(p["kc_of"][l]), int(p["img_of"][l])
            assert kc in (256, 512, 1024)
            if counts[l] > 1:
                assert img >= kc + 2 * L and counts[l] * img <= IMG_BUDGET
    assert muse.window_many_plan(1, L)["launches"] == 1                          # R = 1 is today's single pass


@pytest.mark.parametrize("L", [l for l in PLAN_LS if 1 <= l <= 16])
def test_staged_images_do_not_collide_on_the_lds_banks(muse, L):
    """A ds_read_b64 is served in two groups of 32 lanes (lanes 0-31: the 16 A rows of a tile x the k-lanes q = 0, 1; lanes 32-63:
    q = 2, 3), 64 banks of 4 bytes: inside a group two different doubles collide when they are equal modulo 32.  With the planner's
    image distance no read group of any tile does, whether the tile straddles references or not (both builds: a k-lane is q or
    2 q doubles further on)."""
    W = 2 * L + 1
    p = muse.window_many_plan(muse.window_many_plan(1, L)["max_refs"], L)
    assert p["launches"] == 1
    refs, img, tiles = len(p["launch_of"]), int(p["img_of"][0]), int(p["tiles_of"][0])
    assert refs >= 2
    for qstep in (1, 2):
        for tile in range(tiles):
            for q0 in (0, 2):
                addr = set()
                for q in (q0, q0 + 1):
                    for r in range(16):
                        rr = 16 * tile + r
                        if rr >= refs * W:                 # (the empty rows of the last tile read its last row again)
                            rr = refs * W - 1
                        addr.add((rr // W) * img + rr % W + qstep * q)
                banks = [a % 32 for a in addr]
                assert len(set(banks)) == len(banks), (L, qstep, tile, q0, sorted(addr))
