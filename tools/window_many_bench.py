#!/usr/bin/env python3
"""R references inside a lag window: ONE packed pass (muse_batch_score_many_windowed) against R single-reference windowed passes
(muse_batch_set_lag_window + muse_batch_score per batch: the single-reference kernel, untouched), on resident synthetic groups.

HIP-event time of the scoring launches alone (muse_ctx_kernel_timing: one bracket around the packed pass's launches; the sum of
the R brackets of the separate passes), median of `rounds` after one warm-up round, every (R, L) setting and both forms
alternating inside every round, one process.  Prints ms, the fraction of 8 TB/s on the algorithmic bytes of ONE read of the rows
(8 N + 16 per series), the launches and accumulator tiles of the plan, and separate / packed.
usage: python tools/window_many_bench.py [rounds] [MxN ...]      (default: 7 rounds, the three shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SETTINGS = ((2, 7), (4, 7), (8, 7), (8, 3), (8, 1), (4, 15), (2, 31), (2, 63))
SHAPES = [(1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]


def timed(eng, fn):
    eng.kernel_timing(True)
    fn()
    eng.synchronize()
    ms, _ = eng.kernel_time()
    eng.kernel_timing(False)
    return ms


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    shapes = [tuple(int(v) for v in a.lower().split("x")) for a in sys.argv[2:]] or SHAPES
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs; median of %d per setting after 1 warm-up round, settings and forms alternating" % (name, cus, rounds))
    rmax = max(r for r, _ in SETTINGS)
    for M, N in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        rng = np.random.default_rng(N)
        refs = [ref] + [np.roll(ref, 3 * k) + 0.1 * rng.standard_normal(N) for k in range(1, rmax)]
        dbs = [pkg.DeviceBatch(eng, dg, rf) for rf in refs]
        packed = {s: [] for s in SETTINGS}
        separate = {s: [] for s in SETTINGS}
        names = {}

        def singles(bs, L):
            for b in bs:
                b.set_lag_window(L)
                b.score()
                b.set_lag_window(-1)

        for r in range(rounds + 1):
            for R, L in SETTINGS:
                tp = timed(eng, lambda: pkg.score_many_windowed(dbs[:R], L))
                names[(R, L)] = eng.kernel_name(dbs[0])
                ts = timed(eng, lambda: singles(dbs[:R], L))
                if r > 0:
                    packed[(R, L)].append(tp)
                    separate[(R, L)].append(ts)
        print("%d x %d (n = %d):" % (M, N, dbs[0].n))
        bytes_ = M * (8.0 * N + 16.0)
        for R, L in SETTINGS:
            plan = pkg.window_many_plan(R, min(L, dbs[0].n // 2))
            tp, ts = float(np.median(packed[(R, L)])), float(np.median(separate[(R, L)]))
            print("  R = %d L = %-2d  %-34s launches %d tiles %-9s packed %8.3f ms (min %8.3f)  %5.1f %% of 8 TB/s   %d separate passes %8.3f ms (min %8.3f)   separate / packed %.2f" % (
                R, L, names[(R, L)], plan["launches"], "+".join(str(int(t)) for t in plan["tiles_of"]), tp, float(np.min(packed[(R, L)])),
                bytes_ / (tp * 1e-3) / 8e12 * 100, R, ts, float(np.min(separate[(R, L)])), ts / tp))
        for b in dbs:
            b.close()
        dg.close()
        eng.trim()


if __name__ == "__main__":
    main()
