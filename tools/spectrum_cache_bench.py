#!/usr/bin/env python3
"""The three passes of the spectrum cache on resident synthetic groups, one process, settings alternating.

Per shape and round: the cache is dropped, then
  plain   muse_batch_score with the cache off                      (xcorr_fused_n4096_fold)
  first   the first pass with the cache on: the plain kernel again  (what a group scored once pays: nothing)
  writer  the second pass: allocates the cache and fills it while scoring; its HIP-event time and, beside it, the wall
          time of the whole call behind a synchronisation, hipMalloc included (the one-off cost)
  reader  the third pass                                            (xcorr_cached_n4096)
  reader4 (with `readers`) one more pass with the reader at four workgroups per CU (xcorr_cached_n4096_occ4, a test hook):
          old and new reader alternate in one process, round by round
HIP-event time of the scoring launch (muse_ctx_kernel_timing), median of `rounds` rounds after one warm-up round.  Prints ms,
series/s, the fraction of 8 TB/s on the algorithmic bytes (8 N + 16 per series), and after how many passes over a group the
writer has paid for itself.
usage: python tools/spectrum_cache_bench.py [rounds] [readers] [MxN ...]      (default: 7 rounds, the four shapes of DESIGN 4.10)"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("go-muse_amd")

SHAPES = [(1_000_000, 4096), (200_000, 4096), (65_536, 4096), (400_000, 3000)]
STEPS = ("plain", "first", "writer", "reader")
OLD_READER = "reader4"


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    args = sys.argv[2:]
    steps = STEPS + (OLD_READER,) if "readers" in args else STEPS
    shapes = [tuple(int(v) for v in a.lower().split("x")) for a in args if a != "readers"] or SHAPES
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    print("device %s, %d CUs; median of %d rounds per setting after 1 warm-up round, settings alternating" % (name, cus, rounds))

    def timed(db):
        eng.synchronize()
        eng.kernel_timing(True)
        t0 = time.perf_counter()
        db.score()
        eng.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ms, _ = eng.kernel_time()
        eng.redo_time()
        eng.kernel_timing(False)
        return ms, wall

    for M, N in shapes:
        dg, ref = pkg.DeviceGroup.synthetic(eng, M, N)
        db = pkg.DeviceBatch(eng, dg, ref)
        ev = {s: [] for s in steps}
        wall = {s: [] for s in steps}
        names = {}
        for r in range(rounds + 1):
            dg.drop_spectrum_cache()
            for s in steps:
                eng.set_spectrum_cache(s != "plain")
                eng.spectrum_cache_reader(1 if s == OLD_READER else 0)
                names[s] = eng.kernel_name(db)
                e, w = timed(db)
                if r > 0:
                    ev[s].append(e)
                    wall[s].append(w)
            assert dg.spectrum_cache()[0] == (M & ~1), "the cache was not built: %r" % (dg.spectrum_cache(),)
        eng.set_spectrum_cache(True)
        eng.spectrum_cache_reader(0)
        rows_cached, cache_bytes = dg.spectrum_cache()
        print("%d x %d (n = %d): cache %d rows, %.2f GB" % (M, N, db.n, rows_cached, cache_bytes / 1e9))
        bytes_ = M * (8.0 * N + 16.0)
        med = {s: float(np.median(ev[s])) for s in steps}
        for s in steps:
            t = np.array(ev[s])
            print("  %-7s %-44s median %8.3f ms  min %8.3f ms  %.3e series/s  %5.1f %% of 8 TB/s  x %.2f of plain   call %9.3f ms" % (
                s, names[s] if s != "writer" else "xcorr_cache_fill_n4096", med[s], float(t.min()), M / (med[s] * 1e-3),
                bytes_ / (med[s] * 1e-3) / 8e12 * 100, med["plain"] / med[s], float(np.median(wall[s]))))
        if OLD_READER in steps:
            t_new, t_old = np.array(ev["reader"]), np.array(ev[OLD_READER])
            print("  reader / reader4: median %.3f, new %.3f .. %.3f ms, old %.3f .. %.3f ms" % (
                med["reader"] / med[OLD_READER], float(t_new.min()), float(t_new.max()), float(t_old.min()), float(t_old.max())))
        # passes k >= 3 save (plain - reader) each; pass 2 costs (writer call - plain) once
        extra = float(np.median(wall["writer"])) - float(np.median(wall["plain"]))
        gain = float(np.median(wall["plain"])) - float(np.median(wall["reader"]))
        if gain > 0:
            print("  the writer pass costs %.3f ms more than a plain one (allocation included) and every later pass saves %.3f ms:"
                  " paid for after pass %d over the group" % (extra, gain, 2 + int(np.ceil(extra / gain))))
        else:
            print("  the reader is not faster than the plain kernel here: the cache never pays")
        db.close()
        dg.close()
        eng.trim()


if __name__ == "__main__":
    main()
