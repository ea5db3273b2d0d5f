#!/usr/bin/env python3
"""The masked transform pass of muse_batch_score_in_window against the unwindowed transform pass and against the direct product,
on resident synthetic groups.

Per shape: (a) muse_batch_score with the window off and the spectrum cache off (so both sides read the rows); (b) the masked pass
at L = 7, 31, 63 (forced through the transform kernels: muse_test_in_window_force_transform), 64, 256 and n/2 - 1; (c) the direct
product at L = 7, 31, 63 (float64 groups).  HIP-event time of the scoring launches (muse_ctx_kernel_timing; at n = 4096 the redo
launch behind the fused kernel is reported beside it), median of `rounds` launches after one warm-up round, the settings
alternating inside every round, one process.  Prints ms, (b) / (a) -- the cost of the mask -- and (b) against (c) at equal L.
usage: python tools/in_window_bench.py [rounds] [MxN[f] ...]      (default: 7 rounds, the six shapes of DESIGN 4.9; f = float32 storage)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096, False), (400_000, 3000, False), (2_000_000, 480, False), (1_000_000, 1024, False),
          (500_000, 2048, False), (1_000_000, 4096, True)]
MFMA_LS = (7, 31, 63)


def parse(a):
    f32 = a.lower().endswith("f")
    M, N = (int(v) for v in a.lower().rstrip("f").split("x"))
    return M, N, f32


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    shapes = [parse(a) for a in sys.argv[2:]] or SHAPES
    eng = pkg.get_engine(0)
    B = pkg.binding
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs; median of %d launches per setting after 1 warm-up round, settings alternating" % (name, cus, rounds))
    eng.set_spectrum_cache(False)
    for M, N, f32 in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N, f32=f32)
        db = pkg.DeviceBatch(eng, dg, ref)
        n = db.n
        masked_ls = [L for L in sorted({7, 31, 63, 64, 256, n // 2 - 1}) if L < n // 2]
        settings = [("plain", -1)] + [("masked", L) for L in masked_ls] + ([] if f32 else [("mfma", L) for L in MFMA_LS])
        times = {s: [] for s in settings}
        redo = {s: [] for s in settings}
        names = {}
        for r in range(rounds + 1):
            for s in settings:
                kind, L = s
                eng.in_window_force_transform(kind == "masked")
                eng.kernel_timing(True)
                if kind == "plain":
                    db.score()
                else:
                    db.score_in_window(L)
                    want = B.MUSE_IN_WINDOW_MASKED if kind == "masked" else B.MUSE_IN_WINDOW_MFMA
                    assert db.last_in_window_path() == want, (s, db.last_in_window_path())
                eng.synchronize()
                ms, cnt = eng.kernel_time()
                rms, _ = eng.redo_time()
                eng.kernel_timing(False)
                eng.in_window_force_transform(False)
                names[s] = eng.kernel_name(db)
                if r > 0:
                    times[s].append(ms)
                    redo[s].append(rms)
        print("%d x %d %s (n = %d):" % (M, N, "float32" if f32 else "float64", n))
        med = {s: float(np.median(times[s])) for s in settings}
        plain = med[("plain", -1)]
        for s in settings:
            kind, L = s
            t = np.array(times[s])
            note = ""
            if kind == "masked":
                note = "  (b)/(a) %.3f" % (med[s] / plain)
                if ("mfma", L) in med:
                    note += "  masked / direct product at L = %d: %.2f" % (L, med[s] / med[("mfma", L)])
            print("  %-6s %-9s %-52s median %8.3f ms  min %8.3f ms  redo launch %6.3f ms  %.3e series/s%s" % (
                kind, "" if L < 0 else "L = %d" % L, names[s], med[s], float(t.min()), float(np.median(redo[s])),
                M / (med[s] * 1e-3), note))
        if ("masked", 64) in med and ("mfma", 63) in med:
            print("  ship condition: masked L = 64 %.3f ms %s direct product L = 63 %.3f ms" % (
                med[("masked", 64)], "<" if med[("masked", 64)] < med[("mfma", 63)] else ">=", med[("mfma", 63)]))
        db.close()
        dg.close()
        eng.trim()
    eng.set_spectrum_cache(True)


if __name__ == "__main__":
    main()
