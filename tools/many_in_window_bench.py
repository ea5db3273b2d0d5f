#!/usr/bin/env python3
"""R references inside a wide lag window: ONE masked many-references pass (muse_batch_score_many_in_window) against R consecutive
single masked passes (muse_batch_score_in_window per batch: the code path without this entry point), on resident synthetic groups.

HIP-event time of the scoring launches plus the redo launches behind them (muse_ctx_kernel_timing: kernel time + redo time), median
of `rounds` after one warm-up round, every (R, L) setting and both forms alternating inside every round, one process.  Prints ms,
series-references per second and (a) / (b); the table goes to stdout and to the file given with --out (default
profiles/many_in_window_bench.txt).
usage: python tools/many_in_window_bench.py [--out FILE] [rounds] [MxN[f]:R,R:L,L ...]
       (default: 7 rounds, the shapes of DESIGN 4.9; f = float32 storage)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

# (M, N, float32 storage, the R's, the L's)
SHAPES = [(1_000_000, 4096, False, (4, 8), (64, 256)), (400_000, 3000, False, (8,), (64,)), (1_000_000, 4096, True, (8,), (64,)),
          (2_000_000, 480, False, (4, 8), (64,)), (1_000_000, 1024, False, (4, 8), (64,)), (500_000, 2048, False, (4, 8), (64,))]


def parse(a):
    shape, rs, ls = a.split(":")
    f32 = shape.lower().endswith("f")
    M, N = (int(v) for v in shape.lower().rstrip("f").split("x"))
    return M, N, f32, tuple(int(v) for v in rs.split(",")), tuple(int(v) for v in ls.split(","))


def timed(eng, fn):
    eng.kernel_timing(True)
    fn()
    eng.synchronize()
    ms, _ = eng.kernel_time()
    rms, _ = eng.redo_time()
    eng.kernel_timing(False)
    return ms + rms


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "many_in_window_bench.txt")
    if "--out" in args:
        k = args.index("--out")
        out = args[k + 1]
        args = args[:k] + args[k + 2:]
    rounds = int(args[0]) if args else 7
    shapes = [parse(a) for a in args[1:]] or SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = pkg.get_engine(0)
    B = pkg.binding
    name, cus, hbm = eng.device_info()
    say("device %s, %d CUs; kernel + redo time, median of %d per setting after 1 warm-up round, settings and forms alternating" % (name, cus, rounds))
    say("(a) = R consecutive muse_batch_score_in_window passes; (b) = one muse_batch_score_many_in_window pass")
    for M, N, f32, Rs, Ls in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N, f32=f32)
        rng = np.random.default_rng(N)
        rmax = max(Rs)
        refs = [ref] + [np.roll(ref, 45 * k) + 0.1 * rng.standard_normal(N) for k in range(1, rmax)]
        dbs = [pkg.DeviceBatch(eng, dg, rf) for rf in refs]
        settings = [(R, L) for R in Rs for L in Ls]
        one = {s: [] for s in settings}
        each = {s: [] for s in settings}
        names, plans = {}, {}

        def singles(bs, L):
            for b in bs:
                b.score_in_window(L)

        for r in range(rounds + 1):
            for R, L in settings:
                tb = timed(eng, lambda: pkg.score_many_in_window(dbs[:R], L))
                names[(R, L)] = eng.kernel_name(dbs[0])
                plans[(R, L)] = pkg.many_in_window_plan(N, f32, L, R)
                ta = timed(eng, lambda: singles(dbs[:R], L))
                assert dbs[0].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
                if r > 0:
                    one[(R, L)].append(tb)
                    each[(R, L)].append(ta)
        say("%d x %d %s (n = %d):" % (M, N, "float32" if f32 else "float64", dbs[0].n))
        for R, L in settings:
            tb, ta = float(np.median(one[(R, L)])), float(np.median(each[(R, L)]))
            say("  R = %d L = %-4d plan %d  %-52s (a) %8.3f ms (min %8.3f)  (b) %8.3f ms (min %8.3f)  %.3e series-references/s  (a)/(b) %.2f" % (
                R, L, plans[(R, L)], names[(R, L)], ta, float(np.min(each[(R, L)])), tb, float(np.min(one[(R, L)])),
                M * R / (tb * 1e-3), ta / tb))
        for b in dbs:
            b.close()
        dg.close()
        eng.trim()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
