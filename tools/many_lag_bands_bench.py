#!/usr/bin/env python3
"""Many references, each inside its own lag band and under its own sign, in one pass (muse_batch_score_many_in_lag_bands) against
what a build without it offers for the same questions, on resident synthetic groups.

Per shape, R = 4 and 8 references and the two assignments of ((lo, hi), sign) per reference below, cycled through the references:
  each  the mixed packed pass -- score_many_in_lag_bands(bands, signs): xcorr_window_many_each_mfma, one read of the rows;
  (a)   the R single passes score_in_lag_band(lo_r, hi_r, sign_r), which read the rows R times: what every mirror did when the
        batches' Results differed;
  (b)   the uniform packed pass with the same number of accumulator tiles -- score_many_in_lag_band(1, W, +1) with R references and
        the W that gives those tiles: its answer is another one; the gap to it is the price of the run-time descriptors.
HIP-event time of the scoring launches (muse_ctx_kernel_timing: the sum over the launches of a setting), median of `rounds`
repetitions after one warm-up round, the settings alternating inside every round, one process, the spectrum cache off.  Prints ms
and the ratios, and writes the same lines to profiles/many_lag_bands_bench.txt (or --out PATH).
usage: python tools/many_lag_bands_bench.py [--out PATH] [rounds] [MxN ...]   (default: 7 rounds, the three shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]
RS = (4, 8)
ASSIGNMENTS = (("MIXED", (((1, 7), 0), ((-7, -1), 1), ((1, 16), -1), ((-3, 12), 0), ((1, 1), 1), ((2, 18), 0))),
               ("SYMMETRIC", (((-7, 7), 0), ((-3, 3), -1), ((-15, 15), 1), ((-7, 0), 0))))


def uniform_width(R, tiles):
    """the widest W <= 48 with ceil(R W / 16) == tiles"""
    ws = [w for w in range(1, 49) if (R * w + 15) // 16 == tiles]
    return ws[-1] if ws else None


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "many_lag_bands_bench.txt")
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
        settings, info = [], {}
        for aname, assign in ASSIGNMENTS:
            for R in RS:
                cyc = [assign[r % len(assign)] for r in range(R)]
                bands, signs = [b for b, _ in cyc], [s for _, s in cyc]
                plan = pkg.many_lag_bands_plan(N, False, bands, signs)
                tiles = int(plan["tiles_of"][0])
                Wu = uniform_width(R, tiles) if plan["launches"] == 1 else None
                info[(aname, R)] = (bands, signs, plan, Wu)
                settings += [("each", aname, R), ("single", aname, R)]
                if Wu:
                    settings.append(("uniform", aname, R))

        def run(kind, aname, R):
            bands, signs, plan, Wu = info[(aname, R)]
            if kind == "each":
                pkg.score_many_in_lag_bands(dbs[:R], bands, signs)
            elif kind == "single":
                for b, (lo, hi), s in zip(dbs[:R], bands, signs):
                    b.score_in_lag_band(lo, hi, s)
            else:
                pkg.score_many_in_lag_band(dbs[:R], 1, Wu, 1)
        times = {s: [] for s in settings}
        for r in range(rounds + 1):
            for s in (settings if r % 2 == 0 else settings[::-1]):
                eng.kernel_timing(True)
                run(*s)
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                eng.kernel_timing(False)
                if r > 0:
                    times[s].append(ms)
        say("%d x %d float64 (n = %d):" % (M, N, dbs[0].n))
        med = {s: float(np.median(times[s])) for s in settings}
        for aname, assign in ASSIGNMENTS:
            for R in RS:
                bands, signs, plan, Wu = info[(aname, R)]
                rows = sum(hi - lo + 1 for lo, hi in bands)
                e, a = med[("each", aname, R)], med[("single", aname, R)]
                line = ("  %-9s R = %d  %3d rows  each %8.3f ms (%d launch(es), tiles %s, kc %s)   (a) %d single passes %8.3f ms  (a)/each %5.2f"
                        % (aname, R, rows, e, plan["launches"], "+".join(str(int(t)) for t in plan["tiles_of"]),
                           "+".join(str(int(k)) for k in plan["kc_of"]), R, a, a / e))
                if Wu:
                    u = med[("uniform", aname, R)]
                    line += "   (b) uniform (1, %d) sign +1, the same tiles %8.3f ms  each/(b) %5.3f" % (Wu, u, e / u)
                say(line + "   %.3e series-references/s" % (M * R / (e * 1e-3)))
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
