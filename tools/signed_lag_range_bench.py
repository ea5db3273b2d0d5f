#!/usr/bin/env python3
"""The signed best match (muse_batch_score_signed_in_lag_range) against the unsigned pass of the same path
(muse_batch_score_in_lag_range), on resident synthetic groups, and the unsigned passes against another build of the library.

Part (a), one process: per shape and lag range the three signs 0, +1, -1 -- sign 0 is the unsigned call -- where the dispatch
builds them: (-7, 0), +-15, +-63 on the direct product (float64), +-256 and every lag on the transform kernels (with a sign the
masked kernels; sign 0 at every lag is the plain pass, spectrum cache off, i.e. muse_batch_score's kernel).  HIP-event time of the
scoring launch (muse_ctx_kernel_timing), median of `rounds` launches after one warm-up round, the settings alternating inside
every round.  Prints ms and the ratio signed / unsigned of the same range.
Part (b), with --parent LIB (another build's libmuse_hip.so, e.g. the parent commit's built from a worktree; tools/ab_lib.py's
scheme): the unsigned passes -- score_in_lag_range over the same ranges, score_in_window(63) and the plain all-scores pass -- with
the in-tree library and with LIB, each in its own process, the two alternating, twice; prints both medians and in-tree / other.
Writes the lines to profiles/signed_lag_range_bench.txt (or --out PATH).
usage: python tools/signed_lag_range_bench.py [--out PATH] [--parent LIB] [rounds] [MxN[f] ...]
       (default: 7 rounds; 1000000x4096, 1000000x4096f (float32 storage), 2000000x480, 100000x40000)"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["1000000x4096", "1000000x4096f", "2000000x480", "100000x40000"]
EVERY = 1 << 30
RANGES = ((-7, 0), (-15, 15), (-63, 63), (-256, 256), (-EVERY, EVERY))


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


def rname(lo, hi):
    return "every lag" if hi == EVERY else "[%d, %d]" % (lo, hi)


def measure(pkg, eng, shape, settings, rounds):
    """{setting: (median ms, min ms, kernel name)}; a setting is (call, lo, hi, sign), call in 'range', 'signed', 'window', 'plain'"""
    M, N, f32 = parse(shape)
    dg, ref = pkg.DeviceGroup.synthetic(eng, M, N, f32=f32)
    db = pkg.DeviceBatch(eng, dg, ref)
    times = {s: [] for s in settings}
    names = {}
    for r in range(rounds + 1):
        for s in settings:
            call, lo, hi, sign = s
            eng.kernel_timing(True)
            if call == "plain":
                db.score()
            elif call == "window":
                db.score_in_window(hi)
            elif call == "range":
                db.score_in_lag_range(lo, hi)
            else:
                db.score_signed_in_lag_range(lo, hi, sign)
            eng.synchronize()
            ms, cnt = eng.kernel_time()
            eng.kernel_timing(False)
            names[s] = eng.kernel_name(db)
            if r > 0:
                times[s].append(ms)
    db.close()
    dg.close()
    eng.trim()
    return {s: (float(np.median(times[s])), float(np.min(times[s])), names[s]) for s in settings}


def unsigned_settings(pkg, N, f32):
    B = pkg.binding
    out = [("plain", 0, 0, 0)]
    if pkg.in_window_plan(N, f32, 63) != B.MUSE_IN_WINDOW_UNSUPPORTED:
        out.append(("window", -63, 63, 0))
    out += [("range", lo, hi, 0) for lo, hi in RANGES if pkg.lag_range_plan(N, f32, lo, hi) != B.MUSE_IN_WINDOW_UNSUPPORTED]
    return out


def child(lib, rounds, shapes):
    pkg = load(lib)
    eng = pkg.get_engine(0)
    eng.set_spectrum_cache(False)
    for shape in shapes:
        M, N, f32 = parse(shape)
        res = measure(pkg, eng, shape, unsigned_settings(pkg, N, f32), rounds)
        for s, (med, mn, name) in res.items():
            print("RESULT " + json.dumps([shape, list(s), med, mn, name]), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1] if args[1] != "-" else "", int(args[2]), args[3:])
    out_path = os.path.join(ROOT, "profiles", "signed_lag_range_bench.txt")
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
    say("(a) signed against unsigned, one process")
    eng.set_spectrum_cache(False)
    for shape in shapes:
        M, N, f32 = parse(shape)
        settings = [("plain", 0, 0, 0)]
        for lo, hi in RANGES:
            for sign in (0, 1, -1):
                if pkg.signed_lag_range_plan(N, f32, lo, hi, sign) != B.MUSE_IN_WINDOW_UNSUPPORTED:
                    settings.append(("signed", lo, hi, sign))
        res = measure(pkg, eng, shape, settings, rounds)
        say("%d x %d %s (n = %d):" % (M, N, "float32 storage" if f32 else "float64", pkg.next_pow2(float(N))))
        plain = res[("plain", 0, 0, 0)][0]
        for s in settings:
            call, lo, hi, sign = s
            med, mn, kname = res[s]
            note = ""
            if call == "signed" and sign != 0 and ("signed", lo, hi, 0) in res:
                note = "  signed / unsigned %.3f" % (med / res[("signed", lo, hi, 0)][0])
            if call == "signed" and hi == EVERY and sign != 0:
                note += "  / the unwindowed all-scores pass %.3f" % (med / plain)
            say("  %-11s sign %+d  %-56s median %8.3f ms  min %8.3f ms  %.3e series/s%s" % (
                "all scores" if call == "plain" else rname(lo, hi), sign, kname, med, mn, M / (med * 1e-3), note))
        flush()
    eng.set_spectrum_cache(True)
    del eng
    if parent:
        say("(b) the unsigned passes: in-tree against the other build (--parent), own processes, alternating, two rounds each")
        got = {"in-tree": {}, "other": {}}
        for rnd in range(2):
            for tag, lib in (("in-tree", "-"), ("other", parent)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, str(rounds)] + shapes,
                                     check=True, capture_output=True, text=True).stdout
                for l in out.splitlines():
                    if l.startswith("RESULT "):
                        shape, s, med, mn, kname = json.loads(l[7:])
                        got[tag].setdefault((shape, tuple(s)), []).append((med, kname))
        worst = 0.0
        for key in got["in-tree"]:
            if key not in got["other"]:
                continue
            shape, (call, lo, hi, sign) = key
            a = float(np.median([m for m, _ in got["in-tree"][key]]))
            b = float(np.median([m for m, _ in got["other"][key]]))
            worst = max(worst, a / b)
            what = {"plain": "all scores", "window": "window +-%d" % hi, "range": "range " + rname(lo, hi)}[call]
            say("  %-14s %-22s %-52s in-tree %8.3f ms  other %8.3f ms  in-tree / other %.3f" % (shape, what, got["in-tree"][key][0][1], a, b, a / b))
        say("  ship condition: the slowest unsigned pass takes %.3f of the other build's (the README's box-to-box spread: +-3 %%)" % worst)
        flush()


if __name__ == "__main__":
    main()
