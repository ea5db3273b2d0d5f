#!/usr/bin/env python3
"""Many references inside a one-sided lag range in one pass (muse_batch_score_many_in_lag_range) against the two ways a build
without it answers the same question, on resident synthetic groups.

Per shape, R = 4, 8, 16 references and L = 7, 15, 31: score_many_in_lag_range(-L, 0) and (0, L) -- the references' L + 1 table
rows packed into the accumulator tiles of one matrix product per launch -- against
  (a) R single score_in_lag_range(-L, 0) passes, which read the rows R times, and
  (b) score_many_windowed(L), the symmetric window that contains the range (2 L + 1 rows per reference; its answer is not the
      one-sided one, its time is what the host paid for one read of the rows).
HIP-event time of the scoring launches (muse_ctx_kernel_timing: the sum over the launches of a setting), median of `rounds`
repetitions after one warm-up round, the settings alternating inside every round, one process.  Prints ms and the ratios, and writes
the same lines to profiles/many_lag_range_bench.txt (or --out PATH).
usage: python tools/many_lag_range_bench.py [--out PATH] [rounds] [MxN ...]   (default: 7 rounds, the three shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]
RS = (4, 8, 16)
LS = (7, 15, 31)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "many_lag_range_bench.txt")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    rounds = int(args[0]) if args else 7
    shapes = [tuple(int(v) for v in a.lower().split("x")) for a in args[1:]] or SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    say("device %s, %d CUs; median of %d repetitions per setting after 1 warm-up round, settings alternating" % (name, cus, rounds))
    eng.set_spectrum_cache(False)
    for M, N in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        rng = np.random.default_rng(N)
        dbs = [pkg.DeviceBatch(eng, dg, np.roll(ref, 3 * r) + 0.05 * rng.standard_normal(N)) for r in range(max(RS))]
        run = {"neg": lambda bs, L: pkg.score_many_in_lag_range(bs, -L, 0),
               "pos": lambda bs, L: pkg.score_many_in_lag_range(bs, 0, L),
               "each": lambda bs, L: [b.score_in_lag_range(-L, 0) for b in bs],
               "sym": lambda bs, L: pkg.score_many_windowed(bs, L)}
        settings = [(kind, R, L) for R in RS for L in LS for kind in ("neg", "pos", "each", "sym")]
        times = {s: [] for s in settings}
        for r in range(rounds + 1):
            for s in settings:
                kind, R, L = s
                eng.kernel_timing(True)
                run[kind](dbs[:R], L)
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                eng.kernel_timing(False)
                if r > 0:
                    times[s].append(ms)
        say("%d x %d float64 (n = %d):" % (M, N, dbs[0].n))
        med = {s: float(np.median(times[s])) for s in settings}
        for R in RS:
            for L in LS:
                plan_r = pkg.window_many_plan_rows(R, L + 1)
                plan_s = pkg.window_many_plan(R, L)
                a, b, neg, pos = (med[(k, R, L)] for k in ("each", "sym", "neg", "pos"))
                say("  R = %2d  L = %2d  [-L, 0] %8.3f ms  [0, L] %8.3f ms  (%d launch(es), tiles %s)   (a) %d single ranges %8.3f ms  (a)/many %5.2f"
                    "   (b) many +-L %8.3f ms (%d launch(es), tiles %s)  many/(b) %5.3f   %.3e series-references/s"
                    % (R, L, neg, pos, plan_r["launches"], "+".join(str(int(t)) for t in plan_r["tiles_of"]), R, a, a / neg, b,
                       plan_s["launches"], "+".join(str(int(t)) for t in plan_s["tiles_of"]), neg / b, M * R / (neg * 1e-3)))
        for db in dbs:
            db.close()
        dg.close()
        eng.trim()
    eng.set_spectrum_cache(True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
