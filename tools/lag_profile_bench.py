#!/usr/bin/env python3
"""Lag profiles (muse_batch_lag_profile_device, whole group) against the pass that scans the same lags and returns (lag, mv) alone
(muse_batch_score_in_lag_band, which is muse_batch_score_in_lag_range where the lags hold 0), on resident synthetic groups, in one
process.  The scoring pass is unchanged from the parent commit, so it is the yardstick.

Per shape and band: HIP-event time of the launches (muse_ctx_kernel_timing; a profile of more than 127 lags is several launches,
summed; the table launches are outside the brackets in both), median of `rounds` calls after one warm-up round, the two alternating
inside every round.  Prints ms, the ratio profile / yardstick, and the bytes the profile writes over the bytes the pass reads (W / N).
Then the listed host form, end to end on the host clock: K = 20 series out of the first float64 shape at (-15, 15) -- the call a user
makes after Fetch().
Writes the lines to profiles/lag_profile_bench.txt (or --out PATH).
usage: python tools/lag_profile_bench.py [--out PATH] [rounds] [MxN:lo,hi;lo,hi ...]
       (default: 7 rounds; 1000000x4096 and 2000000x480 at (-7, 7), (-15, 15), (1, 16), (-63, 63); 100000x40000 at (-7, 7), (-63, 63);
        1000000x4096 at (-200, 200): four reads of the rows against the one masked transform pass)"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = "-7,7;-15,15;1,16;-63,63"
SHAPES = ["1000000x4096:" + FOUR + ";-200,200", "2000000x480:" + FOUR, "100000x40000:-7,7;-63,63"]
HOST_K, HOST_BAND = 20, (-15, 15)


def parse(spec):
    shape, bands = spec.split(":")
    M, N = (int(v) for v in shape.lower().split("x"))
    return M, N, [tuple(int(v) for v in b.split(",")) for b in bands.split(";")]


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "lag_profile_bench.txt")
    if args and args[0] == "--out":
        out_path = args[1]
        args = args[2:]
    rounds = int(args[0]) if args else 7
    specs = args[1:] or SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("go-muse_amd")
    import torch
    torch.cuda.init()
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    say("device %s, %d CUs; median of %d calls per setting after 1 warm-up round, the two alternating; spectrum cache off" % (name, cus, rounds))
    eng.set_spectrum_cache(False)
    dev = torch.device("cuda", eng.device)
    host_done = False
    for spec in specs:
        M, N, bands = parse(spec)
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        db = pkg.DeviceBatch(eng, dg, ref)
        say("%d x %d float64 (n = %d):" % (M, N, db.n))
        for lo, hi in bands:
            W = hi - lo + 1
            out = torch.empty((M, W), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            times = {"scan": [], "profile": []}
            kname = ""
            for r in range(rounds + 1):
                for what in ("scan", "profile"):
                    eng.kernel_timing(True)
                    if what == "scan":
                        db.score_in_lag_band(lo, hi, 0)
                    else:
                        pkg.lag_profile_into(db, lo, hi, out)
                    eng.synchronize()
                    ms, cnt = eng.kernel_time()
                    eng.kernel_timing(False)
                    if what == "scan":
                        kname = eng.kernel_name(db)
                    if r > 0:
                        times[what].append(ms)
            a, b = float(np.median(times["scan"])), float(np.median(times["profile"]))
            say("  [%4d, %4d] %3d lags  scan %-46s median %8.3f ms  min %8.3f ms | profile (%d launch%s) median %8.3f ms  min %8.3f ms"
                "  profile / scan %.3f  bytes written / read %.4f" % (
                    lo, hi, W, kname, a, float(np.min(times["scan"])), len(pkg.lag_profile_plan(N, lo, hi)),
                    "" if W <= 127 else "es", b, float(np.min(times["profile"])), b / a, W / N))
            del out
            torch.cuda.empty_cache()
            flush()
        if not host_done:
            host_done = True
            idx = np.random.default_rng(20).choice(M, HOST_K, replace=False).astype(np.int64)
            wall = []
            for r in range(rounds + 1):
                eng.synchronize()
                t0 = time.perf_counter()
                pkg.lag_profile(db, HOST_BAND[0], HOST_BAND[1], idx)
                if r > 0:
                    wall.append((time.perf_counter() - t0) * 1e3)
            say("  host form, %d listed series at (%d, %d), end to end on the host clock: median %.3f ms  min %.3f ms" % (
                HOST_K, HOST_BAND[0], HOST_BAND[1], float(np.median(wall)), float(np.min(wall))))
            flush()
        db.close()
        dg.close()
        eng.trim()
    eng.set_spectrum_cache(True)


if __name__ == "__main__":
    main()
