#!/usr/bin/env python3
"""Many references inside a lag band or under a sign in one pass (muse_batch_score_many_in_lag_band) against what a build without
it offers for the same question, on resident synthetic groups.

Per shape and R = 4, 8, 16 references:
  (a) the packed band -- score_many_in_lag_band(lo, hi) for (1, 7), (1, 15), (-32, -1), (200, 230) -- against R single
      score_in_lag_band(lo, hi) passes, which read the rows R times;
  (b) the packed band against score_many_in_lag_range of the range that contains it ([0, 7], [0, 15], [-32, 0]: one table row more
      per reference; its answer is another one, its time is what the host paid for one read of the rows);
  (c) signed against unsigned over the same range: score_many_in_lag_band(lo, hi, +1) against score_many_in_lag_range(lo, hi), on
      the packed product (the ranges of (b)) and on the masked pass ([0, 255]);
  (d) the masked many-references pass at 256 lags -- the band (1, 256) and the signed range [0, 255] -- against R single masked
      passes of the band (lengths without masked kernels are skipped).
HIP-event time of the scoring launches (muse_ctx_kernel_timing: the sum over the launches of a setting), median of `rounds`
repetitions after one warm-up round, the settings alternating inside every round, one process, the spectrum cache off.  Prints ms
and the ratios, and writes the same lines to profiles/many_lag_band_bench.txt (or --out PATH).
usage: python tools/many_lag_band_bench.py [--out PATH] [rounds] [MxN ...]   (default: 7 rounds, the three shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]
RS = (4, 8, 16)
BANDS = (((1, 7), (0, 7)), ((1, 15), (0, 15)), ((-32, -1), (-32, 0)), ((200, 230), None))   # (band, the range that contains it)
MASKED_BAND, MASKED_RANGE = (1, 256), (0, 255)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "many_lag_band_bench.txt")
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
        masked = pkg.many_lag_band_plan(N, False, MASKED_BAND[0], MASKED_BAND[1], 0, 2) != 0
        run = {"band": lambda bs, w: pkg.score_many_in_lag_band(bs, w[0], w[1], 0),
               "each": lambda bs, w: [b.score_in_lag_band(w[0], w[1], 0) for b in bs],
               "range": lambda bs, w: pkg.score_many_in_lag_range(bs, w[0], w[1]),
               "pos": lambda bs, w: pkg.score_many_in_lag_band(bs, w[0], w[1], 1)}
        settings = []
        for R in RS:
            for band, rng_ in BANDS:
                settings += [("band", R, band), ("each", R, band)]
                if rng_:
                    settings += [("range", R, rng_), ("pos", R, rng_)]
            if masked:
                settings += [("band", R, MASKED_BAND), ("each", R, MASKED_BAND), ("range", R, MASKED_RANGE), ("pos", R, MASKED_RANGE)]
        times = {s: [] for s in settings}
        for r in range(rounds + 1):
            for s in settings:
                kind, R, w = s
                eng.kernel_timing(True)
                run[kind](dbs[:R], w)
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                eng.kernel_timing(False)
                if r > 0:
                    times[s].append(ms)
        say("%d x %d float64 (n = %d):" % (M, N, dbs[0].n))
        med = {s: float(np.median(times[s])) for s in settings}
        for R in RS:
            for band, rng_ in BANDS:
                Wd = band[1] - band[0] + 1
                plan = pkg.window_many_plan_rows(R, Wd)
                b, e = med[("band", R, band)], med[("each", R, band)]
                line = ("  R = %2d  band (%d, %d)  W = %2d  many %8.3f ms (%d launch(es), tiles %s)   (a) %d single bands %8.3f ms  (a)/many %5.2f"
                        % (R, band[0], band[1], Wd, b, plan["launches"], "+".join(str(int(t)) for t in plan["tiles_of"]), R, e, e / b))
                if rng_:
                    g, p = med[("range", R, rng_)], med[("pos", R, rng_)]
                    line += ("   (b) many range [%d, %d] %8.3f ms  band/(b) %5.3f   (c) the range under sign +1 %8.3f ms  signed/unsigned %5.3f"
                             % (rng_[0], rng_[1], g, b / g, p, p / g))
                say(line + "   %.3e series-references/s" % (M * R / (b * 1e-3)))
            if masked:
                b, e = med[("band", R, MASKED_BAND)], med[("each", R, MASKED_BAND)]
                g, p = med[("range", R, MASKED_RANGE)], med[("pos", R, MASKED_RANGE)]
                say("  R = %2d  masked, 256 lags (plan %d): (d) many band (1, 256) %8.3f ms  %d single bands %8.3f ms  single/many %5.2f"
                    "   (c) many range [0, 255] %8.3f ms  under sign +1 %8.3f ms  signed/unsigned %5.3f  %d single/signed many %5.2f"
                    % (R, pkg.many_lag_band_plan(N, False, MASKED_BAND[0], MASKED_BAND[1], 0, R), b, R, e, e / b, g, p, p / g, R, e / p))
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
