#!/usr/bin/env python3
"""The lag-window pass against the transform pass of the same build, on resident synthetic groups.

Times muse_batch_score with the window off and with L = 7, 15, 31, 63: HIP-event time of the scoring launch alone
(muse_ctx_kernel_timing; with the window off the redo launch behind the fused kernel is reported beside it), median of
`rounds` launches after one warm-up round, off and on alternating inside every round, one process.  Prints ms, series/s and
the fraction of 8 TB/s on the algorithmic bytes (8 N + 16 per series).
usage: python tools/window_bench.py [rounds] [MxN ...]      (default: 7 rounds, the five shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

WINDOWS = (-1, 7, 15, 31, 63)
SHAPES = [(1_000_000, 4096), (2_000_000, 480), (200_000, 5000), (100_000, 40000), (50_000, 65536)]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    shapes = [tuple(int(v) for v in a.lower().split("x")) for a in sys.argv[2:]] or SHAPES
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs; median of %d launches per setting after 1 warm-up round, settings alternating" % (name, cus, rounds))
    for M, N in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        db = pkg.DeviceBatch(eng, dg, ref)
        times = {L: [] for L in WINDOWS}
        redo = []
        names = {}
        for r in range(rounds + 1):
            for L in WINDOWS:
                db.set_lag_window(L)
                names[L] = eng.kernel_name(db)
                eng.kernel_timing(True)
                db.score()
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                rms, _ = eng.redo_time()
                eng.kernel_timing(False)
                if r > 0:
                    times[L].append(ms)
                    if L < 0:
                        redo.append(rms)
        db.set_lag_window(-1)
        print("%d x %d (n = %d):" % (M, N, db.n))
        bytes_ = M * (8.0 * N + 16.0)
        off = float(np.median(times[-1]))
        for L in WINDOWS:
            t = np.array(times[L])
            med = float(np.median(t))
            print("  %-10s %-44s median %9.3f ms  min %9.3f ms  %.3e series/s  %5.1f %% of 8 TB/s  x %.2f of the transform pass%s" % (
                "off" if L < 0 else "L = %d" % L, names[L], med, float(t.min()), M / (med * 1e-3), bytes_ / (med * 1e-3) / 8e12 * 100,
                off / med, "  (+ redo launch %.3f ms)" % float(np.median(redo)) if L < 0 else ""))
        db.close()
        dg.close()
        eng.trim()


if __name__ == "__main__":
    main()
