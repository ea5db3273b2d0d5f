"""Rows that are already resident, against the host path (DESIGN.md section "Resident rows").

  1. append_from: a sub-group of 50 000 rows picked at random (sorted, as FilterByLabelValues returns them) out of 1 000 000
     resident rows, gathered HBM -> HBM (row_gather.hip), plain and non-temporal stores; TB/s counted as read + write.
     Against: the same number of rows uploaded from a packed host array (DeviceGroup.append, the host mirror's path with
     reuse off).  N = 4096, 480 and an odd length (4095).
  2. Muse.Run: run_group_rows (rows named in a resident group) against run_rows (the rows from host memory) at the reference's
     BenchmarkMuseRunLarge shape (100 graphs x 50 series x 480 samples, 16 callers on one template) and at 20 000 x 4096
     (one caller).

Wall-clock medians over several repetitions, each ended by a wait for the device.  One JSON line per measurement, and a
summary table at the end.  Usage: python tools/resident_bench.py [--quick] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pkg():
    import importlib
    return importlib.import_module("go-muse_amd")


def _median_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def bench_append_from(muse, eng, N, src_rows, sub_rows, reps, emit):
    src, _ = muse.DeviceGroup.synthetic(eng, src_rows, N, seed=N)
    rng = np.random.default_rng(N)
    idx = np.sort(rng.choice(src_rows, size=sub_rows, replace=False))
    nbytes = sub_rows * N * 8
    for nt in (False, True):
        eng.gather_nontemporal(nt)
        t = []
        for r in range(reps + 1):
            dst = muse.DeviceGroup(eng, N, sub_rows)   # (capacity reserved: the timed call grows nothing)
            eng.synchronize()
            t0 = time.perf_counter()
            dst.append_from(src, idx)
            dst.read(0, 1)   # (the gather runs on the copy stream: a read waits for both streams)
            if r:
                t.append((time.perf_counter() - t0) * 1e3)
            if r == reps:   # spot check of the last gather
                assert np.array_equal(dst.read(17, 1)[0], src.read(int(idx[17]), 1)[0])
            dst.close()
        med = statistics.median(t)
        emit({"what": "append_from", "N": N, "rows": sub_rows, "of": src_rows, "nontemporal": nt, "ms": med, "best_ms": min(t),
              "TBps_rw": 2 * nbytes / (med * 1e-3) / 1e12})
    eng.gather_nontemporal(False)

    host = np.random.default_rng(1).standard_normal((sub_rows, N))

    def upload():
        g = muse.DeviceGroup(eng, N, sub_rows)
        g.append(host)
        eng.synchronize()
        g.close()

    med, best = _median_ms(upload, max(2, reps // 2))
    emit({"what": "host_upload", "N": N, "rows": sub_rows, "ms": med, "best_ms": best, "GBps": nbytes / (med * 1e-3) / 1e9})
    src.close()


def bench_muse_run(muse, eng, N, src_rows, graph_rows, graphs, callers, reps, emit, label):
    src, ref = muse.DeviceGroup.synthetic(eng, src_rows, N, seed=7 + N)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), ref)
    rng = np.random.default_rng(3)
    lists = [np.sort(rng.choice(src_rows, size=graph_rows, replace=False)) for _ in range(graphs)]
    host_all = src.read(0, src_rows) if src_rows * N <= (1 << 28) else None
    host = [host_all[l] if host_all is not None else np.random.default_rng(k).standard_normal((graph_rows, N))
            for k, l in enumerate(lists)]
    per = (graphs + callers - 1) // callers

    def run(resident):
        def work(t):
            for k in range(t * per, min(graphs, (t + 1) * per)):
                if resident:
                    tmpl.run_group_rows(src, lists[k])
                else:
                    tmpl.run_rows(host[k])
        if callers == 1:
            work(0)
        else:
            th = [threading.Thread(target=work, args=(t,)) for t in range(callers)]
            for x in th:
                x.start()
            for x in th:
                x.join()

    for resident in (True, False):
        med, best = _median_ms(lambda: run(resident), reps)
        emit({"what": "muse_run", "shape": label, "path": "run_group_rows" if resident else "run_rows", "N": N,
              "graphs": graphs, "rows_per_graph": graph_rows, "callers": callers, "ms": med, "best_ms": best})
    if host_all is not None:
        for k in range(min(graphs, 5)):
            a, b = tmpl.run_group_rows(src, lists[k]), tmpl.run_rows(host[k])
            assert a[1] == b[1] and int(a[0]["series"]) == int(b[0]["series"]) and a[0]["score"] == b[0]["score"]
    tmpl.close()
    src.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="smaller source groups and fewer repetitions")
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
    src_rows = 200_000 if a.quick else 1_000_000
    reps = 3 if a.quick else 7
    for N in (4096, 480, 4095):
        bench_append_from(muse, eng, N, src_rows, 50_000, reps, emit)
    bench_muse_run(muse, eng, 480, 5000, 50, 100, 16, reps, emit, "BenchmarkMuseRunLarge 100 x 50 x 480, 16 callers")
    bench_muse_run(muse, eng, 4096, src_rows, 20_000, 1, 1, reps, emit, "20000 x 4096, one caller")

    summary = ["", "%-48s %10s %10s" % ("measurement", "median ms", "rate")]
    for d in lines:
        if d.get("what") == "append_from":
            summary.append("%-48s %10.3f %7.2f TB/s" % ("append_from N=%d %s" % (d["N"], "nt" if d["nontemporal"] else "plain"),
                                                        d["ms"], d["TBps_rw"]))
        elif d.get("what") == "host_upload":
            summary.append("%-48s %10.3f %7.1f GB/s" % ("host upload N=%d" % d["N"], d["ms"], d["GBps"]))
        elif d.get("what") == "muse_run":
            summary.append("%-48s %10.3f" % ("%s: %s" % (d["shape"][:30], d["path"]), d["ms"]))
    print("\n".join(summary))
    if out:
        out.write("\n".join(summary) + "\n")
        out.close()


if __name__ == "__main__":
    main()
