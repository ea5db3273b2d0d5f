#!/usr/bin/env python3
"""Lag bands (muse_batch_score_in_lag_band) against the lag range that contains them (muse_batch_score_signed_in_lag_range), on
resident synthetic groups, and the unchanged passes against another build of the library.

Part (a), one process: per shape the pairs band / range
    (1, 16) / (0, 16), (32, 63) / (0, 63), (64, 126) / (0, 126)   the direct product: 1 / 2, 2 / 4 and 4 / 8 accumulator tiles
    (200, 230) / (0, 230)                                         a band far from zero: two tiles against the masked transform pass
    (1, 256) / (0, 256), (100, 300) / (0, 300)                    both on the masked transform pass, signs 0, +1 and -1
where the dispatch builds them (a float32-storage shape runs everything on the masked pass).  HIP-event time of the scoring launches
(muse_ctx_kernel_timing), median of `rounds` launches after one warm-up round, the settings alternating inside every round.  Prints
ms and the ratio band / range.
Part (b), with --parent LIB (another build's libmuse_hip.so, e.g. the parent commit's; tools/ab_lib.py's scheme): the plain all-scores
pass (bench.py's headline step) and score_in_lag_range(-63, 63), with the in-tree library and with LIB, each in its own process, the
two alternating, three times each; prints both medians and in-tree / other, and whether the scores the two builds leave are the same
bytes.
Writes the lines to profiles/lag_band_bench.txt (or --out PATH).
usage: python tools/lag_band_bench.py [--out PATH] [--parent LIB] [rounds] [MxN[f] ...]
       (default: 7 rounds; 1000000x4096, 1000000x4096f (float32 storage), 2000000x480, 100000x40000)"""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["1000000x4096", "1000000x4096f", "2000000x480", "100000x40000"]
PAIRS = (((1, 16), (0, 16), (0,)), ((32, 63), (0, 63), (0,)), ((64, 126), (0, 126), (0,)), ((200, 230), (0, 230), (0,)),
         ((1, 256), (0, 256), (0, 1, -1)), ((100, 300), (0, 300), (0, 1, -1)))


def parse(shape):
    f32 = shape.endswith("f")
    M, N = (int(v) for v in shape.rstrip("f").lower().split("x"))
    return M, N, f32


def load(lib):
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("go-muse_amd")
    if lib:
        import ctypes
        pkg.build.LIB = lib
        pkg.build.stale = lambda: False
        L = ctypes.CDLL(lib)
        pkg.binding.SIGNATURES = {k: v for k, v in pkg.binding.SIGNATURES.items() if hasattr(L, k)}   # (an older build lacks newer entry points)
    return pkg


def measure(pkg, eng, shape, settings, rounds, digest=False):
    """{setting: (median ms, min ms, kernel name[, sha1 of the scores])}; a setting is (call, lo, hi, sign), call in 'band', 'range',
    'plain'"""
    M, N, f32 = parse(shape)
    dg, ref = pkg.DeviceGroup.synthetic(eng, M, N, f32=f32)
    db = pkg.DeviceBatch(eng, dg, ref)
    times = {s: [] for s in settings}
    names, sums = {}, {}
    for r in range(rounds + 1):
        for s in settings:
            call, lo, hi, sign = s
            eng.kernel_timing(True)
            if call == "plain":
                db.score()
            elif call == "band":
                db.score_in_lag_band(lo, hi, sign)
            else:
                db.score_signed_in_lag_range(lo, hi, sign)
            eng.synchronize()
            ms, cnt = eng.kernel_time()
            eng.kernel_timing(False)
            names[s] = eng.kernel_name(db)
            if r > 0:
                times[s].append(ms)
            if digest and r == rounds:
                lag, mv = db.read_scores()
                sums[s] = hashlib.sha1(lag.tobytes() + mv.tobytes()).hexdigest()[:16]
    db.close()
    dg.close()
    eng.trim()
    return {s: (float(np.median(times[s])), float(np.min(times[s])), names[s], sums.get(s, "")) for s in settings}


def child(lib, rounds, shapes):
    pkg = load(lib)
    eng = pkg.get_engine(0)
    eng.set_spectrum_cache(False)
    for shape in shapes:
        M, N, f32 = parse(shape)
        settings = [("plain", 0, 0, 0)]
        if pkg.lag_range_plan(N, f32, -63, 63) != pkg.binding.MUSE_IN_WINDOW_UNSUPPORTED:
            settings.append(("range", -63, 63, 0))
        for s, (med, mn, name, sha) in measure(pkg, eng, shape, settings, rounds, digest=True).items():
            print("RESULT " + json.dumps([shape, list(s), med, mn, name, sha]), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1] if args[1] != "-" else "", int(args[2]), args[3:])
    out_path = os.path.join(ROOT, "profiles", "lag_band_bench.txt")
    parent = ""
    while args and args[0] in ("--out", "--parent"):
        if args[0] == "--out":
            out_path = args[1]
        else:
            parent = os.path.abspath(args[1])
        args = args[2:]
    rounds = int(args[0]) if args else 7
    shapes = args[1:] or SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")

    pkg = load("")
    B = pkg.binding
    eng = pkg.get_engine(0)
    name, cus, hbm = eng.device_info()
    say("device %s, %d CUs; median of %d launches per setting after 1 warm-up round, settings alternating; spectrum cache off" % (name, cus, rounds))
    say("(a) a band against the range that contains it, one process")
    eng.set_spectrum_cache(False)
    paths = {B.MUSE_IN_WINDOW_MFMA: "direct", B.MUSE_IN_WINDOW_MASKED: "masked"}
    for shape in shapes:
        M, N, f32 = parse(shape)
        settings = []
        for band, rng, signs in PAIRS:
            for sign in signs:
                try:
                    pb = pkg.lag_band_plan(N, f32, band[0], band[1], sign)
                except pkg.MuseError:
                    continue                                         # (nothing of the band is left at this length)
                pr = pkg.signed_lag_range_plan(N, f32, rng[0], rng[1], sign)
                if pb != B.MUSE_IN_WINDOW_UNSUPPORTED:
                    settings.append(("band", band[0], band[1], sign))
                if pr != B.MUSE_IN_WINDOW_UNSUPPORTED:
                    settings.append(("range", rng[0], rng[1], sign))
        res = measure(pkg, eng, shape, settings, rounds)
        say("%d x %d %s (n = %d):" % (M, N, "float32 storage" if f32 else "float64", pkg.next_pow2(float(N))))
        for band, rng, signs in PAIRS:
            for sign in signs:
                kb, kr = ("band", band[0], band[1], sign), ("range", rng[0], rng[1], sign)
                for k in (kr, kb):
                    if k not in res:
                        continue
                    med, mn, kname, _ = res[k]
                    note = "  band / range %.3f" % (med / res[kr][0]) if k is kb and kr in res else ""
                    say("  %-5s [%4d, %4d] sign %+d  %-50s median %8.3f ms  min %8.3f ms  %.3e series/s%s" % (
                        k[0], k[1], k[2], sign, kname, med, mn, M / (med * 1e-3), note))
        flush()
    eng.set_spectrum_cache(True)
    del eng
    if parent:
        say("(b) the unchanged passes: in-tree against the other build (--parent), own processes, alternating, three rounds each")
        got = {"in-tree": {}, "other": {}}
        for rnd in range(3):
            for tag, lib in (("in-tree", "-"), ("other", parent)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(rounds)] + shapes,
                                     check=True, capture_output=True, text=True).stdout
                for l in out.splitlines():
                    if l.startswith("RESULT "):
                        shape, s, med, mn, kname, sha = json.loads(l[7:])
                        got[tag].setdefault((shape, tuple(s)), []).append((med, kname, sha))
        worst, same = 0.0, True
        for key in got["in-tree"]:
            if key not in got["other"]:
                continue
            shape, (call, lo, hi, sign) = key
            a = float(np.median([m for m, _, _ in got["in-tree"][key]]))
            b = float(np.median([m for m, _, _ in got["other"][key]]))
            worst = max(worst, a / b)
            eq = len({h for _, _, h in got["in-tree"][key] + got["other"][key]}) == 1
            same = same and eq
            what = "all scores" if call == "plain" else "range [%d, %d]" % (lo, hi)
            say("  %-14s %-16s %-44s in-tree %8.3f ms  other %8.3f ms  in-tree / other %.3f  scores %s" % (
                shape, what, got["in-tree"][key][0][1], a, b, a / b, "identical" if eq else "DIFFER"))
        say("  the slowest of them takes %.3f of the other build's (the README's box-to-box spread: +-3 %%); dumped scores %s" % (
            worst, "identical everywhere" if same else "DIFFER"))
        flush()


if __name__ == "__main__":
    main()
