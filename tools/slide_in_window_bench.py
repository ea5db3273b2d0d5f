#!/usr/bin/env python3
"""muse_batch_slide_score_in_window at FFT length 4096 (the SLIDE builds of xcorr_fused_n4096_fold): the slide of a resident group and
the transform pass over the new rows in ONE kernel, against the two kernels it replaces, on resident synthetic groups (DESIGN.md
section 4.9, "The slide inside the n = 4096 transform pass").

For every listed (shape, storage, k, L):
  (a) kernel time: the HIP-event time of the fused kernel (muse_ctx_kernel_timing brackets its launch) against the sum of the row
      slide kernel's and the pass kernel's brackets of the same call with TWO_STEP forced (muse_test_slide_in_window_force: the
      parent commit's kernels), the same rows, the same process.  Bytes over HBM: 2 x elem N M against 3 x elem N M.
  (b) wall clock of one fused call (tails packed into pinned memory, sent, the wait for the device, the kernel) against
      DeviceGroup.slide + score_in_window + synchronize.

One box, one process; median of 7 after one warm-up round; the forms and the cases of a shape (k, L) alternate inside a round, so
none of them sits on a warmer or cooler box than the others.  The group's spectrum cache is off (the stand-alone unwindowed pass
would otherwise count towards one; no form here reads it).  One JSON line per measurement and a summary table at the end.
Usage: python tools/slide_in_window_bench.py [--quick] [--out FILE]
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

# (M, N, float32 storage, ((k, L), ...)); L = 2048 = n/2: the unwindowed pass
SHAPES = [(400_000, 4096, False, ((16, 2048), (16, 256), (1, 2048))),
          (400_000, 4096, True, ((16, 2048),)),
          (400_000, 3000, False, ((16, 2048),)),
          (1_000_000, 4096, False, ((16, 2048),))]
FORMS = ("fused", "two_step", "calls")


def _pkg():
    import importlib
    return importlib.import_module("go-muse_amd")


def bench_shape(muse, eng, M, N, f32, cases, reps, emit):
    B = muse.binding
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=N + M, f32=f32)
    db = muse.DeviceBatch(eng, dg, ref)
    rng = np.random.default_rng(N)
    tails = {k: rng.standard_normal((M, k)) for k in sorted({k for k, _ in cases})}
    t = {(f, c): {"kern": [], "wall": []} for f in FORMS for c in cases}
    parts = {c: {"slide": [], "pass": []} for c in cases}
    names = {}
    eng.kernel_timing(True)
    eng.kernel_time()
    for r in range(reps + 1):                    # round 0 warms up (tails' buffers, score buffers, the kernels' code)
        for ci, (k, L) in enumerate(cases):
            order = FORMS[(r + ci) % 3:] + FORMS[:(r + ci) % 3]
            for form in order:
                eng.synchronize()
                t0 = time.perf_counter()
                if form == "fused":
                    db.slide_score_in_window(tails[k], L)
                    t1 = time.perf_counter()
                    ms, launches = eng.kernel_time()
                    assert launches == 1 and db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_FUSED
                    names[(k, L)] = eng.kernel_name(db)
                elif form == "two_step":
                    eng.slide_in_window_force(1)
                    db.slide_score_in_window(tails[k], L)
                    t1 = time.perf_counter()
                    eng.slide_in_window_force(0)
                    ms, launches = eng.kernel_time()
                    assert launches == 2 and db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
                else:
                    dg.slide(tails[k])
                    ms_slide, launches = eng.kernel_time()
                    assert launches == 1
                    db.score_in_window(L)
                    eng.synchronize()
                    t1 = time.perf_counter()
                    ms_pass, launches = eng.kernel_time()
                    assert launches == 1
                    ms = ms_slide + ms_pass
                    if r:
                        parts[(k, L)]["slide"].append(ms_slide)
                        parts[(k, L)]["pass"].append(ms_pass)
                if r:
                    t[(form, (k, L))]["kern"].append(ms)
                    t[(form, (k, L))]["wall"].append((t1 - t0) * 1e3)
    eng.kernel_timing(False)
    elem = 4 if f32 else 8
    for c in cases:
        k, L = c
        med = {f: (statistics.median(t[(f, c)]["kern"]), statistics.median(t[(f, c)]["wall"])) for f in FORMS}
        fk = med["fused"][0]
        emit({"what": "slide_in_window", "M": M, "N": N, "f32": f32, "k": k, "L": L, "kernel": names[c],
              "fused_kernel_ms": fk, "fused_kernel_best_ms": min(t[("fused", c)]["kern"]),
              "fused_TBps_rw": 2.0 * elem * N * M / (fk * 1e-3) / 1e12,
              "two_step_kernels_ms": med["two_step"][0], "two_step_kernels_best_ms": min(t[("two_step", c)]["kern"]),
              "slide_kernel_ms": statistics.median(parts[c]["slide"]), "pass_kernel_ms": statistics.median(parts[c]["pass"]),
              "calls_kernels_ms": med["calls"][0], "kernel_ratio": med["two_step"][0] / fk, "bytes_ratio_ceiling": 1.5,
              "fused_call_ms": med["fused"][1], "two_step_call_ms": med["two_step"][1], "two_calls_ms": med["calls"][1],
              "call_ratio": med["calls"][1] / med["fused"][1], "tail_MB": M * k * elem / 1e6})
    for h in (db, dg):
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
    eng.set_spectrum_cache(False)
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
    for M, N, f32, cases in SHAPES:
        if a.quick:
            M //= 10
        if 1.2 * M * N * (4 if f32 else 8) > hbm * 0.9:
            emit({"what": "skipped", "M": M, "N": N, "why": "does not fit in device memory"})
            continue
        bench_shape(muse, eng, M, N, f32, cases, reps, emit)

    summary = ["", "%-18s %-7s %3s %5s | %9s %9s | %9s %9s %9s %7s | %10s %10s %7s" % (
        "shape", "storage", "k", "L", "fused ms", "TB/s r+w", "slide ms", "pass ms", "2-step ms", "x fused", "fused call", "two calls",
        "x fused")]
    for d in lines:
        if d.get("what") != "slide_in_window":
            continue
        summary.append("%-18s %-7s %3d %5d | %9.3f %9.2f | %9.3f %9.3f %9.3f %7.2f | %10.2f %10.2f %7.2f" % (
            "%d x %d" % (d["M"], d["N"]), "float32" if d["f32"] else "float64", d["k"], d["L"], d["fused_kernel_ms"],
            d["fused_TBps_rw"], d["slide_kernel_ms"], d["pass_kernel_ms"], d["two_step_kernels_ms"], d["kernel_ratio"],
            d["fused_call_ms"], d["two_calls_ms"], d["call_ratio"]))
    summary.append("(2-step ms: the two kernels of the same call with the fused kernel switched off; by bytes the ceiling is 1.50 x)")
    print("\n".join(summary))
    if out:
        out.write("\n".join(summary) + "\n")
        out.close()


if __name__ == "__main__":
    main()
