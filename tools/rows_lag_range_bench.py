#!/usr/bin/env python3
"""Muse.Run inside a lag range (muse_batch_run_rows_in_lag_range; xcorr_window_panels.hip) measured on one box.

All figures but the wall clocks of (c) are the HIP-event time of the SCORING launches of one call (muse_ctx_kernel_timing: the
bracket around launch_window, the split's or the panels' partial + finish launches, or the transform kernel) over rows resident
in a group and scored where they lie.  Median of `rounds` after one warm-up round, the settings alternating inside every round.

(a) No regression: run_group_rows_windowed at L = 7 / 31 / 63 on 100 x 40000 and 1000 x 4096, this tree's library against another
    build's (--parent <libmuse_hip.so>: the parent commit's), each in a process of its own, the two alternating five times.  The
    tree's medians must lie inside the range of the parent's own five medians (widened by its own spread on either side).
(b) The panel path: 16 and 100 rows x 4096, 16384, 40000 (100 rows) and 65536 (16 rows) samples at W = 255, 1025 and 2048 lags (the
    range -(W // 2) .. W - 1 - W // 2), the planner's S against 1, the powers of two, half, twice and four times of it and one-chunk
    slices; beside it the unwindowed run_group_rows of the same rows.  window_panels_plan ships the rule this part supports.
(c) 1000 x 4096, the same W: the panel path against the one other way to the same answer -- upload + score_in_lag_range through the
    masked transform pass (event time of its scoring launches, and wall clock of upload + batch + pass against the wall clock of
    run_rows_in_lag_range over the same host rows).  Measured: the masked pass WINS there at every W (24 us against 63 ... 367 us of
    scoring launches, and the whole call from host rows too); slot rows are not routed to it.

usage: python tools/rows_lag_range_bench.py [rounds] [--parent other.so] [abc]     -> profiles/rows_lag_range_bench.txt"""
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGRESS_SHAPES = [(100, 40000), (1000, 4096)]
REGRESS_WINDOWS = (7, 31, 63)
PANEL_SHAPES = [(100, 40000), (16, 65536), (16, 4096), (100, 4096), (16, 16384), (100, 16384)]
WIDTHS = (255, 1025, 2048)
WIN_KC = 1024


def load(lib=None):
    pkg = importlib.import_module("go-muse_amd")
    if lib:
        import ctypes
        pkg.build.LIB = lib
        pkg.build.stale = lambda: False
        L = ctypes.CDLL(lib)
        pkg.binding.SIGNATURES = {k: v for k, v in pkg.binding.SIGNATURES.items() if hasattr(L, k)}   # (an older build lacks newer entry points)
    return pkg


def rows_of(M, N, seed):
    rng = np.random.default_rng(seed)
    ref = np.zeros(N)
    ref[N // 2 - N // 40:N // 2 + N // 40] = 2.0
    ref += 0.1 * rng.standard_normal(N)
    rows = np.empty((M, N))
    for r in range(M):
        rows[r] = np.roll(ref, int(rng.integers(-1000, 1001))) + 0.3 * rng.standard_normal(N)
    return ref, rows


def timed(eng, call):
    eng.kernel_timing(True)
    call()
    eng.synchronize()
    ms, cnt = eng.kernel_time()
    eng.kernel_timing(False)
    return ms * 1e3


def span_of(W):
    return -(W // 2), W - 1 - W // 2


def child_regress(lib, rounds):
    """one process, one library: the medians of run_group_rows_windowed, one line per (shape, L)"""
    pkg = load(lib)
    eng = pkg.get_engine(0)
    for M, N in REGRESS_SHAPES:
        ref, rows = rows_of(M, N, 7 * M + N)
        src = pkg.DeviceGroup.from_rows(eng, rows)
        probe = pkg.DeviceGroup(eng, N, 0)
        tmpl = pkg.DeviceBatch(eng, probe, ref)
        at = np.arange(M, dtype=np.int64)
        t = {L: [] for L in REGRESS_WINDOWS}
        for r in range(rounds + 1):
            for L in REGRESS_WINDOWS:
                us = timed(eng, lambda: tmpl.run_group_rows_windowed(src, at, L))
                if r > 0:
                    t[L].append(us)
        for L in REGRESS_WINDOWS:
            print("R %d %d %d %.3f %.3f %.3f" % (M, N, L, float(np.median(t[L])), float(np.min(t[L])), float(np.max(t[L]))), flush=True)
        tmpl.close()
        probe.close()
        src.close()


def regress(parent, rounds):
    print("(a) run_group_rows_windowed, us: median of %d after 1 warm-up round per process, L alternating; this tree and the parent's "
          "library in processes of their own, alternating five times" % rounds)
    if not parent:
        print("  (no --parent library given: skipped)")
        return True
    got = {"tree": {}, "parent": {}}
    for rep in range(5):
        for tag, lib in (("parent", parent), ("tree", "")):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-regress", lib, str(rounds)], check=True,
                                 capture_output=True, text=True).stdout
            for l in out.splitlines():
                if l.startswith("R "):
                    f = l.split()
                    got[tag].setdefault((int(f[1]), int(f[2]), int(f[3])), []).append(float(f[4]))
    ok = True
    for key in sorted(got["parent"]):
        p, t = got["parent"][key], got["tree"][key]
        spread = max(p) - min(p)
        lo, hi = min(p) - spread, max(p) + spread
        inside = all(lo <= x <= hi for x in t)
        ok = ok and inside
        print("  %5d x %-6d L = %-2d parent %s  tree %s  tree / parent (medians) %.3f  %s" % (
            key[0], key[1], key[2], " ".join("%8.1f" % x for x in p), " ".join("%8.1f" % x for x in t),
            float(np.median(t)) / float(np.median(p)), "inside the parent's range" if inside else "OUTSIDE the parent's range"))
    return ok


def candidates(planned, chunks):
    return sorted({1, max(1, planned // 2), planned, min(chunks, 2 * planned), min(chunks, 4 * planned), chunks} |
                  {S for S in (2, 4, 8, 16, 32) if S <= chunks})


def panels(pkg, eng, rounds):
    cus = eng.device_info()[1]
    print("(b) the panel path, us: median of %d after 1 warm-up round, S alternating; rows resident, scored where they lie" % rounds)
    for M, N in PANEL_SHAPES:
        chunks = (N + WIN_KC - 1) // WIN_KC
        ref, rows = rows_of(M, N, 7 * M + N)
        src = pkg.DeviceGroup.from_rows(eng, rows)
        probe = pkg.DeviceGroup(eng, N, 0)
        tmpl = pkg.DeviceBatch(eng, probe, ref)
        at = np.arange(M, dtype=np.int64)
        plain = []
        for r in range(rounds + 1):
            us = timed(eng, lambda: tmpl.run_group_rows(src, at))
            if r > 0:
                plain.append(us)
        print("  %5d x %-6d unwindowed run_group_rows %8.1f us" % (M, N, float(np.median(plain))))
        for W in WIDTHS:
            lo, hi = span_of(W)
            path, pn, planned = pkg.rows_lag_range_plan(M, N, cus, lo, hi)
            Ss = candidates(planned, chunks)
            t = {S: [] for S in Ss}
            for r in range(rounds + 1):
                for S in Ss:
                    eng.window_rows_slices(S)
                    us = timed(eng, lambda: tmpl.run_group_rows_in_lag_range(src, at, lo, hi))
                    if r > 0:
                        t[S].append(us)
            eng.window_rows_slices(0)
            best = min(Ss, key=lambda S: float(np.median(t[S])))
            line = "  %5d x %-6d W = %-4d blocks %2d panels %2d chunks %2d planner S = %-2d fastest S = %-2d |" % (
                M, N, W, (M + 15) // 16, pn, chunks, planned, best)
            for S in Ss:
                line += "  S=%-2d %8.1f us" % (S, float(np.median(t[S])))
            flops = 2.0 * M * N * W
            line += "  | planner: %.1f Tflop/s of the window's 2 M N W, x %.2f of the unwindowed pass" % (
                flops / (float(np.median(t[planned])) * 1e-6) / 1e12, float(np.median(t[planned])) / float(np.median(plain)))
            print(line)
        tmpl.close()
        probe.close()
        src.close()
        eng.trim()


def masked(pkg, eng, rounds):
    M, N = 1000, 4096
    cus = eng.device_info()[1]
    print("(c) %d x %d: the panel path against upload + score_in_lag_range through the masked transform pass; median of %d after 1 "
          "warm-up round, the two alternating" % (M, N, rounds))
    ref, rows = rows_of(M, N, 7 * M + N)
    src = pkg.DeviceGroup.from_rows(eng, rows)
    db = pkg.DeviceBatch(eng, src, ref)
    probe = pkg.DeviceGroup(eng, N, 0)
    tmpl = pkg.DeviceBatch(eng, probe, ref)
    at = np.arange(M, dtype=np.int64)
    for W in WIDTHS:
        lo, hi = span_of(W)
        path, pn, planned = pkg.rows_lag_range_plan(M, N, cus, lo, hi)
        ev = {"panels": [], "masked": []}
        wall = {"panels": [], "masked": []}

        def upload_and_score():
            dg = pkg.DeviceGroup.from_rows(eng, rows)
            b = pkg.DeviceBatch.like(tmpl, dg)
            b.score_in_lag_range(lo, hi)
            eng.synchronize()
            b.close()
            dg.close()
        for r in range(rounds + 1):
            a = timed(eng, lambda: tmpl.run_group_rows_in_lag_range(src, at, lo, hi))
            b = timed(eng, lambda: db.score_in_lag_range(lo, hi))
            t0 = time.perf_counter()
            tmpl.run_rows_in_lag_range(rows, lo, hi)
            t1 = time.perf_counter()
            upload_and_score()
            t2 = time.perf_counter()
            if r > 0:
                ev["panels"].append(a)
                ev["masked"].append(b)
                wall["panels"].append((t1 - t0) * 1e3)
                wall["masked"].append((t2 - t1) * 1e3)
        print("  W = %-4d panels %2d S = %-2d | scoring launches: panels %8.1f us, masked pass %8.1f us (x %.2f) | wall clock from host rows: "
              "run_rows_in_lag_range %7.3f ms, upload + score_in_lag_range %7.3f ms" % (
                  W, pn, planned, float(np.median(ev["panels"])), float(np.median(ev["masked"])),
                  float(np.median(ev["panels"])) / float(np.median(ev["masked"])), float(np.median(wall["panels"])),
                  float(np.median(wall["masked"]))))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child-regress":
        child_regress(args[1], int(args[2]))
        return 0
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    rounds = int(args[0]) if args and args[0].isdigit() else 7
    parts = args[-1] if args and not args[-1].isdigit() else "abc"
    ok = True
    if "a" in parts:
        ok = regress(parent, rounds)
    pkg = load()
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs" % (name, cus))
    if "b" in parts:
        panels(pkg, eng, rounds)
    if "c" in parts:
        masked(pkg, eng, rounds)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
