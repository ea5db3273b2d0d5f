"""muse_group_slide (row_slide.hip): a resident group follows time in place, against freeing it and uploading it again
("Rows that follow time").

For every shape M x N (float64 rows generated in HBM) and k in {1, 16, 64} -- 8-byte and 16-byte units:
  (a) the HIP-event time of the slide kernel alone (muse_ctx_kernel_timing brackets its launch), as bytes moved per second
      (2 x 8 x N x M: every row is read and written once).  Yardstick: the row gather (row_gather.hip, append_from of the same
      rows in order into a second group: the same read-plus-write pattern) timed in the same process by the wall clock of the
      call plus a wait for the copy stream.
  (b) the wall clock of the whole call (tails packed into pinned memory, sent, the wait for the device, the kernel), against the
      only alternative without it: muse_group_free + an upload of the slid rows from host memory (DeviceGroup.append of a packed
      host array).

One box, one process; median of 7 after one warm-up round, the settings (k = 1, 16, 64) alternating inside a round.  One JSON line
per measurement and a summary table at the end.  Usage: python tools/slide_bench.py [--quick] [--out FILE]
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

KS = (1, 16, 64)


def _pkg():
    import importlib
    return importlib.import_module("go-muse_amd")


def _host_bytes_available():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                return int(ln.split()[1]) * 1024
    except OSError:
        pass
    return os.sysconf("SC_PHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")


def bench_shape(muse, eng, M, N, reps, upload_reps, emit):
    nbytes = M * N * 8
    dg, _ = muse.DeviceGroup.synthetic(eng, M, N, seed=N + M)
    rng = np.random.default_rng(N)
    tails = {k: rng.standard_normal((M, k)) for k in KS}
    wall = {k: [] for k in KS}
    kern = {k: [] for k in KS}
    eng.kernel_timing(True)
    eng.kernel_time()
    for r in range(reps + 1):                   # round 0 warms up (the tails' buffers are allocated there)
        for k in KS:
            eng.synchronize()
            t0 = time.perf_counter()
            dg.slide(tails[k])                  # (returns when the rows have moved)
            t1 = time.perf_counter()
            ms, launches = eng.kernel_time()
            assert launches == 1
            if r:
                wall[k].append((t1 - t0) * 1e3)
                kern[k].append(ms)
    eng.kernel_timing(False)
    probe = dg.read(M - 1, 1)[0]                # spot check: the last row ends with the tails of the last three slides
    assert np.array_equal(probe[-64:], tails[64][M - 1]) and np.array_equal(probe[-80:-64], tails[16][M - 1])
    for k in KS:
        km, wm = statistics.median(kern[k]), statistics.median(wall[k])
        emit({"what": "slide", "M": M, "N": N, "k": k, "unit_bytes": 16 if k % 2 == 0 and N % 2 == 0 else 8, "kernel_ms": km,
              "kernel_best_ms": min(kern[k]), "kernel_TBps_rw": 2 * nbytes / (km * 1e-3) / 1e12, "call_ms": wm, "call_best_ms": min(wall[k]),
              "tail_MB": M * k * 8 / 1e6})

    # the yardstick: the same rows gathered in order into a second group
    idx = np.arange(M, dtype=np.int64)
    t = []
    for r in range(reps + 1):
        dst = muse.DeviceGroup(eng, N, M)       # (capacity reserved: the timed call grows nothing)
        eng.synchronize()
        t0 = time.perf_counter()
        dst.append_from(dg, idx)
        dst.read(0, 1)                          # (the gather runs on the copy stream: a read waits for both streams)
        if r:
            t.append((time.perf_counter() - t0) * 1e3)
        dst.close()
    gm = statistics.median(t)
    emit({"what": "gather", "M": M, "N": N, "call_ms": gm, "call_best_ms": min(t), "TBps_rw": 2 * nbytes / (gm * 1e-3) / 1e12})

    # the alternative: free the group and upload the slid rows from host memory
    host = dg.read(0, M) if nbytes < 0.4 * _host_bytes_available() else None
    if host is None:
        emit({"what": "skipped", "M": M, "N": N, "why": "the host copy for the upload does not fit in host memory"})
    else:
        t = []
        for r in range(upload_reps + 1):
            eng.synchronize()
            t0 = time.perf_counter()
            dg.close()
            dg = muse.DeviceGroup(eng, N, M)
            dg.append(host)
            eng.synchronize()
            if r:
                t.append((time.perf_counter() - t0) * 1e3)
        um = statistics.median(t)
        emit({"what": "free_and_upload", "M": M, "N": N, "call_ms": um, "call_best_ms": min(t), "GBps": nbytes / (um * 1e-3) / 1e9})
        del host
    dg.close()
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
    shapes = [(400_000, 4096), (1_000_000, 4096), (2_000_000, 480), (100_000, 40000)]
    reps, upload_reps = (3, 2) if a.quick else (7, 3)
    for M, N in shapes:
        if a.quick:
            M //= 10
        if 3 * M * N * 8 > hbm * 0.9:           # the group, the gather's second group and the tails beside the rest
            emit({"what": "skipped", "M": M, "N": N, "why": "does not fit in device memory beside the gather's second group"})
            continue
        bench_shape(muse, eng, M, N, reps, upload_reps, emit)

    by = {(d["what"], d["M"], d["N"], d.get("k")): d for d in lines if "what" in d and d["what"] != "skipped"}
    summary = ["", "%-22s %3s %5s | %9s %9s %8s | %9s %11s %8s" % ("shape", "k", "unit", "kernel ms", "TB/s r+w", "x gather", "call ms",
                                                                "upload ms", "x upload")]
    for d in lines:
        if d.get("what") != "slide":
            continue
        g, u = by.get(("gather", d["M"], d["N"], None)), by.get(("free_and_upload", d["M"], d["N"], None))
        summary.append("%-22s %3d %4dB | %9.3f %9.2f %8.2f | %9.3f %11s %8s" % (
            "%d x %d" % (d["M"], d["N"]), d["k"], d["unit_bytes"], d["kernel_ms"], d["kernel_TBps_rw"],
            d["kernel_TBps_rw"] / g["TBps_rw"] if g else float("nan"), d["call_ms"],
            "%.1f" % u["call_ms"] if u else "-", "%.1f" % (u["call_ms"] / d["call_ms"]) if u else "-"))
    summary.append("")
    for d in lines:
        if d.get("what") == "gather":
            summary.append("gather of the same rows, %d x %d: %.3f ms (wall clock of the call), %.2f TB/s read + write" % (
                d["M"], d["N"], d["call_ms"], d["TBps_rw"]))
        elif d.get("what") == "free_and_upload":
            summary.append("free + upload from host memory, %d x %d: %.1f ms, %.1f GB/s" % (d["M"], d["N"], d["call_ms"], d["GBps"]))
    print("\n".join(summary))
    if out:
        out.write("\n".join(summary) + "\n")
        out.close()


if __name__ == "__main__":
    main()
