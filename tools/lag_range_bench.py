#!/usr/bin/env python3
"""One-sided lag ranges (muse_batch_score_in_lag_range) against the symmetric window that contains them (muse_batch_score_in_window),
on resident synthetic groups.

Per shape and L = 7, 15, 31, 63: score_in_window(L) -- at equal arguments the code path of the build without lag ranges --
against score_in_lag_range(-L, 0) and (0, L) on the direct product (half the lag rows: ceil((L + 1) / 16) accumulator tiles
instead of ceil((2 L + 1) / 16)); where the length has masked kernels also score_in_window(256) against
score_in_lag_range(-256, 0) (the mask's cost is constant; at n = 512, where +-256 is every lag and runs WITHOUT a mask, also
against the widest masked window +-255).  HIP-event time of the scoring launch (muse_ctx_kernel_timing), median
of `rounds` launches after one warm-up round, the settings alternating inside every round, one process.  Prints ms and the ratio
one-sided / symmetric, and writes the same lines to profiles/lag_range_bench.txt (or --out PATH).
usage: python tools/lag_range_bench.py [--out PATH] [rounds] [MxN ...]      (default: 7 rounds, the three shapes of DESIGN 4.9)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]
LS = (7, 15, 31, 63)
WIDE = 256


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "lag_range_bench.txt")
    if args and args[0] == "--out":
        out_path, args = args[1], args[2:]
    rounds = int(args[0]) if args else 7
    shapes = [tuple(int(v) for v in a.lower().split("x")) for a in args[1:]] or SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = pkg.get_engine(0)
    B = pkg.binding
    name, cus, hbm = eng.device_info()
    say("device %s, %d CUs; median of %d launches per setting after 1 warm-up round, settings alternating" % (name, cus, rounds))
    eng.set_spectrum_cache(False)
    for M, N in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        db = pkg.DeviceBatch(eng, dg, ref)
        n = db.n
        settings = []
        for L in LS:
            settings += [("sym", -L, L), ("neg", -L, 0), ("pos", 0, L)]
        masked_sym = None
        if pkg.lag_range_plan(N, False, -WIDE, 0) == B.MUSE_IN_WINDOW_MASKED:
            settings += [("sym", -WIDE, WIDE), ("neg", -WIDE, 0)]
            if pkg.in_window_plan(N, False, WIDE) == B.MUSE_IN_WINDOW_PLAIN:
                # n = 512: +-256 is every lag, the pass WITHOUT a mask; the widest masked window shows what the mask itself costs
                masked_sym = ("sym", -(n // 2 - 1), n // 2 - 1)
                settings.append(masked_sym)
        times = {s: [] for s in settings}
        names = {}
        for r in range(rounds + 1):
            for s in settings:
                kind, lo, hi = s
                eng.kernel_timing(True)
                if kind == "sym":
                    db.score_in_window(hi)
                else:
                    db.score_in_lag_range(lo, hi)
                # (the direct product up to 127 lags, the masked pass beyond; n = 512: +-256 is every lag, the plain pass)
                want = pkg.in_window_plan(N, False, hi) if kind == "sym" else pkg.lag_range_plan(N, False, lo, hi)
                assert db.last_in_window_path() == want != B.MUSE_IN_WINDOW_UNSUPPORTED, (s, db.last_in_window_path())
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                eng.kernel_timing(False)
                names[s] = eng.kernel_name(db)
                if r > 0:
                    times[s].append(ms)
        say("%d x %d float64 (n = %d):" % (M, N, n))
        med = {s: float(np.median(times[s])) for s in settings}
        worst = 0.0
        for s in settings:
            kind, lo, hi = s
            t = np.array(times[s])
            note = ""
            if kind != "sym":
                L = max(-lo, hi)
                ratio = med[s] / med[("sym", -L, L)]
                note = "  one-sided / symmetric %.3f" % ratio
                if L == WIDE and masked_sym:
                    ratio = med[s] / med[masked_sym]
                    note += " (the unmasked pass); / the masked +-%d %.3f" % (masked_sym[2], ratio)
                worst = max(worst, ratio)
            say("  [%5d, %4d] %-52s median %8.3f ms  min %8.3f ms  %.3e series/s%s" % (
                lo, hi, names[s], med[s], float(t.min()), M / (med[s] * 1e-3), note))
        say("  ship condition: the slowest one-sided range takes %.3f of its symmetric window of the same pass (must stay within 1.03)" % worst)
        db.close()
        dg.close()
        eng.trim()
    eng.set_spectrum_cache(True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
