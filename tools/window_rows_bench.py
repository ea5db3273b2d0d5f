#!/usr/bin/env python3
"""The windowed Muse.Run (muse_batch_run_rows_windowed; xcorr_window_split.hip) measured two ways, one process, one box.

(a) Wall clock of ONE call: Muse.RunWindowed (the Python mirror) and the ABI call alone (muse_batch_run_rows_windowed on packed
    rows) against what a caller had to do before the entry point existed for the same answer: muse_group_upload,
    muse_batch_create_like, muse_batch_set_lag_window, muse_batch_run_groups with G = 1, then the two frees.
    Shapes 50 x 480, 100 x 4096, 100 x 40000, 500 x 65536, 20000 x 4096 (the last two exceed a slot: the general path), L = 7, 31.
(b) HIP-event time of the SCORING launches of one call (muse_ctx_kernel_timing: the bracket around launch_window, or around the
    partial + finish launches of the split) over rows resident in a group and scored where they lie, forced S = 1 against every
    slice count a planner with a minimum of 1, 2, 4 or 8 chunks per slice would pick (and half of it), from 16 x 4096 up to the
    largest groups a slot takes (2^24 samples: 256 x 65536, 4096 x 4096).

Protocol of tools/window_bench.py: median of `rounds` after one warm-up round, the settings alternating inside every round.
usage: python tools/window_rows_bench.py [rounds] [a|b]      (default: 7 rounds, both parts) -> profiles/window_rows_bench.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

WALL_SHAPES = [(50, 480), (100, 4096), (100, 40000), (500, 65536), (20000, 4096)]
EVENT_SHAPES = [(16, 4096), (100, 4096), (1000, 4096), (4096, 4096), (16, 16384), (100, 16384), (1000, 16384), (16, 40000),
                (100, 40000), (400, 40000), (16, 65536), (100, 65536), (256, 65536)]
WINDOWS = (7, 31)
WIN_KC = 1024


def rows_of(M, N, seed):
    rng = np.random.default_rng(seed)
    ref = np.zeros(N)
    ref[N // 2 - N // 40:N // 2 + N // 40] = 2.0
    ref += 0.1 * rng.standard_normal(N)
    rows = np.empty((M, N))
    for r in range(M):
        rows[r] = np.roll(ref, int(rng.integers(-100, 101))) + 0.3 * rng.standard_normal(N)
    return ref, rows


def wall(eng, rounds):
    print("(a) wall clock of one call, ms: median of %d after 1 warm-up round, the three forms alternating" % rounds)
    for M, N in WALL_SHAPES:
        ref, rows = rows_of(M, N, M + N)
        series = [pkg.NewSeries(rows[i], pkg.NewLabels({"i": str(i)})) for i in range(M)]
        gid = np.zeros(M, dtype=np.int32)
        for L in WINDOWS:
            res = pkg.NewResults(L, 5, 0.0, pkg.SignFilter_ANY)
            m = pkg.New(pkg.NewSeries(ref, None), res, engine=eng)
            tmpl = m._template

            def mirror():
                m.RunWindowed(series)
                return None

            def abi():
                return tmpl.run_rows_windowed(rows, L)

            def before():
                dg = pkg.DeviceGroup.from_rows(eng, rows)
                db = pkg.DeviceBatch.like(tmpl, dg)
                db.set_lag_window(L)
                rec, state = db.run_groups(gid, 1, 0, abs_scores=False)
                db.close()
                dg.close()
                return rec[0], int(state[0])
            forms = (("Muse.RunWindowed", mirror), ("run_rows_windowed", abi), ("upload+like+set_lag_window+run_groups", before))
            t = {k: [] for k, _ in forms}
            out = {}
            for r in range(rounds + 1):
                for k, f in forms:
                    t0 = time.perf_counter()
                    out[k] = f()
                    dt = time.perf_counter() - t0
                    if r > 0:
                        t[k].append(dt * 1e3)
            a, b = out["run_rows_windowed"], out["upload+like+set_lag_window+run_groups"]
            same = int(a[0]["series"]) == int(b[0]["series"]) and int(a[0]["lag"]) == int(b[0]["lag"]) and a[1] == b[1]
            S, cps = pkg.window_rows_plan(M, N, eng.device_info()[1])
            base = float(np.median(t["upload+like+set_lag_window+run_groups"]))
            print("  %6d x %-6d L = %-2d planner S = %-2d same winner: %s" % (M, N, L, S if M * N <= 1 << 24 else 1, same))
            for k, _ in forms:
                med = float(np.median(t[k]))
                print("      %-40s median %9.3f ms  min %9.3f ms  x %.2f" % (k, med, float(np.min(t[k])), base / med))
            res.Fetch()
        eng.trim()


def candidates(M, N, cus):
    blocks = (M + 15) // 16
    chunks = (N + WIN_KC - 1) // WIN_KC
    out = {1}
    if blocks < cus:
        for min_cps in (1, 2, 4, 8):
            S = max(1, min(cus // blocks, chunks // min_cps))
            out.add(S)
            out.add(max(1, S // 2))
    return sorted(out)


def events(eng, rounds):
    cus = eng.device_info()[1]
    print("(b) HIP-event time of the scoring launches of one call, us: median of %d after 1 warm-up round, S alternating; rows resident, "
          "scored where they lie" % rounds)
    for M, N in EVENT_SHAPES:
        ref, rows = rows_of(M, N, 7 * M + N)
        src = pkg.DeviceGroup.from_rows(eng, rows)
        probe = pkg.DeviceGroup(eng, N, 0)
        tmpl = pkg.DeviceBatch(eng, probe, ref)
        at = np.arange(M, dtype=np.int64)
        for L in WINDOWS:
            Ss = candidates(M, N, cus)
            t = {S: [] for S in Ss}
            for r in range(rounds + 1):
                for S in Ss:
                    eng.window_rows_slices(S)
                    eng.kernel_timing(True)
                    tmpl.run_group_rows_windowed(src, at, L)
                    eng.synchronize()
                    ms, cnt = eng.kernel_time()
                    eng.kernel_timing(False)
                    if r > 0:
                        t[S].append(ms * 1e3)
            eng.window_rows_slices(0)
            one = float(np.median(t[1]))
            plan = pkg.window_rows_plan(M, N, cus)[0]
            line = "  %5d x %-6d L = %-2d blocks %3d chunks %2d planner S = %-2d |" % (M, N, L, (M + 15) // 16, (N + WIN_KC - 1) // WIN_KC, plan)
            for S in Ss:
                med = float(np.median(t[S]))
                line += "  S=%-2d %8.1f us (x %.2f)" % (S, med, one / med)
            print(line)
        tmpl.close()
        probe.close()
        src.close()
        eng.trim()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    parts = sys.argv[2] if len(sys.argv) > 2 else "ab"
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs" % (name, cus))
    if "b" in parts:
        events(eng, rounds)
    if "a" in parts:
        wall(eng, rounds)


if __name__ == "__main__":
    main()
