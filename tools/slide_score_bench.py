#!/usr/bin/env python3
"""muse_batch_slide_score_windowed (xcorr_window_slide.hip): the slide of a resident group and the windowed pass over the new rows
in ONE kernel, against the two calls it replaces (muse_group_slide, then muse_batch_set_lag_window + muse_batch_score), on resident
synthetic groups ("The slide and the windowed pass in one kernel").

For every shape M x N and window L, with k = 16 (16-byte units) and k = 1 (8-byte units):
  (a) kernel time: the HIP-event time of the fused kernel (muse_ctx_kernel_timing brackets its launch) against the sum of the slide
      kernel's and the windowed pass's, the same rows, the same process.  Bytes: 2 x 8 N M against 3 x 8 N M.
  (b) wall clock of one fused call (tails packed into pinned memory, sent, the wait for the device, the kernel) against
      DeviceGroup.slide + set_lag_window + score + synchronize.

One box, one process; median of 7 after one warm-up round; the two forms and the two k alternate inside a round, so neither form
and neither unit width sits on a warmer or cooler box than the other.  One JSON line per measurement and a summary table at the end.
Usage: python tools/slide_score_bench.py [--quick] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (16, 1)
SHAPES = [(400_000, 4096, (7, 15, 31)), (1_000_000, 4096, (7, 15, 31)), (2_000_000, 480, (7,)), (100_000, 40000, (7,))]


def _pkg():
    import importlib
    return importlib.import_module("go-muse_amd")


def bench_shape(muse, eng, M, N, windows, reps, emit):
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=N + M)
    fused = muse.DeviceBatch(eng, dg, ref)       # its own window stays off: the window is the call's argument
    pair = muse.DeviceBatch(eng, dg, ref)        # the two-call form's batch
    rng = np.random.default_rng(N)
    tails = {k: rng.standard_normal((M, k)) for k in KS}
    for L in windows:
        pair.set_lag_window(L)
        t = {(f, k): {"kern": [], "wall": []} for f in ("fused", "pair") for k in KS}
        parts = {k: {"slide": [], "window": []} for k in KS}
        eng.kernel_timing(True)
        eng.kernel_time()
        for r in range(reps + 1):                # round 0 warms up (tables, tails' buffers, score buffers)
            for k in KS:
                for form in (("fused", "pair") if r % 2 else ("pair", "fused")):
                    eng.synchronize()
                    t0 = time.perf_counter()
                    if form == "fused":
                        fused.slide_score_windowed(tails[k], L)
                        t1 = time.perf_counter()
                        ms, launches = eng.kernel_time()
                        assert launches == 1
                    else:
                        dg.slide(tails[k])
                        ms_slide, launches = eng.kernel_time()
                        assert launches == 1
                        pair.score()
                        eng.synchronize()
                        t1 = time.perf_counter()
                        ms_win, launches = eng.kernel_time()
                        assert launches == 1
                        ms = ms_slide + ms_win
                        if r:
                            parts[k]["slide"].append(ms_slide)
                            parts[k]["window"].append(ms_win)
                    if r:
                        t[(form, k)]["kern"].append(ms)
                        t[(form, k)]["wall"].append((t1 - t0) * 1e3)
        eng.kernel_timing(False)
        for k in KS:
            f, p = t[("fused", k)], t[("pair", k)]
            fk, pk = statistics.median(f["kern"]), statistics.median(p["kern"])
            fw, pw = statistics.median(f["wall"]), statistics.median(p["wall"])
            emit({"what": "slide_score", "M": M, "N": N, "k": k, "L": L, "kernel": eng.kernel_name(pair),
                  "fused_kernel_ms": fk, "fused_kernel_best_ms": min(f["kern"]), "fused_TBps_rw": 2 * 8.0 * N * M / (fk * 1e-3) / 1e12,
                  "slide_kernel_ms": statistics.median(parts[k]["slide"]), "window_kernel_ms": statistics.median(parts[k]["window"]),
                  "pair_kernel_ms": pk, "pair_kernel_best_ms": min(p["kern"]), "kernel_ratio": pk / fk,
                  "fused_call_ms": fw, "pair_call_ms": pw, "call_ratio": pw / fw, "tail_MB": M * k * 8 / 1e6})
    # spot check: both forms left the same kind of rows behind -- the last row ends with the last tails that went in
    probe = dg.read(M - 1, 1)[0]
    assert np.array_equal(probe[-1:], tails[1][M - 1])
    for h in (fused, pair, dg):
        h.close()
    eng.trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the rows and 3 repetitions")
    ap.add_argument("--out", default=None, help="also write the JSON lines and the summary here")
    a = ap.parse_args()
    muse = _pkg()
    muse.build.build()
    eng = muse.get_engine(0)
    lines = []
    out = open(a.out, "w") if a.out else None

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(d)
        if out:
            out.write(s + "\n")
            out.flush()

    name, cus, hbm = eng.device_info()
    emit({"device": name, "cus": cus})
    reps = 3 if a.quick else 7
    for M, N, windows in SHAPES:
        if a.quick:
            M //= 10
        if 1.2 * M * N * 8 > hbm * 0.9:
            emit({"what": "skipped", "M": M, "N": N, "why": "does not fit in device memory"})
            continue
        bench_shape(muse, eng, M, N, windows, reps, emit)

    summary = ["", "%-20s %3s %3s | %9s %9s | %9s %9s %9s %7s | %9s %9s %7s" % (
        "shape", "k", "L", "fused ms", "TB/s r+w", "slide ms", "window ms", "sum ms", "x fused", "fused call", "two calls", "x fused")]
    for d in lines:
        if d.get("what") != "slide_score":
            continue
        summary.append("%-20s %3d %3d | %9.3f %9.2f | %9.3f %9.3f %9.3f %7.2f | %9.2f %9.2f %7.2f" % (
            "%d x %d" % (d["M"], d["N"]), d["k"], d["L"], d["fused_kernel_ms"], d["fused_TBps_rw"], d["slide_kernel_ms"],
            d["window_kernel_ms"], d["pair_kernel_ms"], d["kernel_ratio"], d["fused_call_ms"], d["pair_call_ms"], d["call_ratio"]))
    print("\n".join(summary))
    if out:
        out.write("\n".join(summary) + "\n")
        out.close()


if __name__ == "__main__":
    main()
