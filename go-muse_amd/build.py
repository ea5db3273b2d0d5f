"""Builds go-muse_amd/lib/libmuse_hip.so (gfx950 only) with hipcc.

The library is built IN-TREE so it travels with the repo snapshot to the GPU
box; it is git-ignored.  hipcc cross-compiles gfx950 code objects without a
GPU present.
"""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "libmuse_hip.so")
SOURCES = ["xcorr_kernels.hip", "xcorr_r16_fold.hip", "xcorr_r16_cached.hip", "xcorr_r16_occ4.hip", "xcorr_stockham.hip", "xcorr_two_sided.hip", "xcorr_small.hip", "xcorr_long.hip", "xcorr_real.hip", "xcorr_huge.hip", "xcorr_r16_screen.hip", "xcorr_screen_stk.hip", "reduce_kernels.hip", "diag_kernels.hip", "capi_context.hip", "capi_group.hip", "capi_batch.hip", "capi_run.hip", "capi_rows.hip", "capi_screen.hip", "capi_many.hip", "capi_huge.hip", "capi_xcorr.hip", "row_gather.hip", "row_slide.hip", "xcorr_window.hip", "xcorr_window_band.hip", "xcorr_window_profile.hip", "capi_window.hip", "capi_profile.hip", "xcorr_window_many.hip", "capi_window_many.hip", "capi_window_many_in.hip", "xcorr_window_many_band.hip", "capi_window_many_band.hip", "xcorr_window_many_each.hip", "capi_window_many_each.hip", "xcorr_window_split.hip", "xcorr_window_slide.hip", "xcorr_window_panels.hip"]
HEADERS = [os.path.join(CSRC, "xcorr_kernels.h"), os.path.join(CSRC, "xcorr_huge.h"), os.path.join(CSRC, "fft_device.h"), os.path.join(CSRC, "r16_device.h"), os.path.join(CSRC, "fold_device.h"), os.path.join(CSRC, "foldk_device.h"), os.path.join(CSRC, "n4096_pair_device.h"), os.path.join(CSRC, "long_device.h"), os.path.join(CSRC, "stk_device.h"), os.path.join(CSRC, "small_device.h"), os.path.join(CSRC, "xcorr_small_body.h"), os.path.join(CSRC, "two_device.h"), os.path.join(CSRC, "window_device.h"), os.path.join(CSRC, "capi_internal.h"), os.path.join(ROOT, "include", "muse_hip.h"), os.path.join(ROOT, "include", "muse_hip_test.h")]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


# per-source extra flags: the fp32 screening kernel must keep scalar fp32 ops (2-cycle
# issue); SLP packing into v_pk_*_f32 costs v_mov shuffles and issues no faster
PER_FILE_FLAGS = {"xcorr_r16_screen.hip": ["-fno-slp-vectorize"], "xcorr_screen_stk.hip": ["-fno-slp-vectorize"]}


def build(force=False, verbose=False, extra_flags=()):
    if not force and not stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    base = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + list(extra_flags)
    objs = []
    for src in SOURCES:
        obj = os.path.join(objdir, src + ".o")
        cmd = base + PER_FILE_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        objs.append(obj)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("-") and a != "--force"]
    print(build(force=True, verbose=True, extra_flags=flags))


def _build_host_program(name, opt, force):
    """g++ build of host/<name>.cpp, a program over the C++ host mirror (host/muse.hpp), linked to libmuse_hip.so."""
    src = os.path.join(PKG, "host", name + ".cpp")
    hdr = os.path.join(PKG, "host", "muse.hpp")
    exe = os.path.join(LIBDIR, name)
    build()
    if (not force and os.path.exists(exe)
            and os.path.getmtime(exe) >= max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(LIB))):
        return exe
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), src, "-o", exe,
                           "-L" + LIBDIR, "-lmuse_hip", "-pthread", "-Wl,-rpath," + LIBDIR])
    return exe


HOST_TEST = os.path.join(LIBDIR, "muse_host_test")
REF_BENCH = os.path.join(LIBDIR, "muse_ref_bench")
COLD_PHASES = os.path.join(LIBDIR, "muse_cold_phases")
RESIDENT_TEST = os.path.join(LIBDIR, "muse_resident_test")
WINDOW_TEST = os.path.join(LIBDIR, "muse_window_test")
WINDOW_MANY_TEST = os.path.join(LIBDIR, "muse_window_many_test")
ROWS_WINDOW_TEST = os.path.join(LIBDIR, "muse_rows_window_test")
IN_WINDOW_TEST = os.path.join(LIBDIR, "muse_in_window_test")
MANY_IN_WINDOW_TEST = os.path.join(LIBDIR, "muse_many_in_window_test")
LAG_RANGE_TEST = os.path.join(LIBDIR, "muse_lag_range_test")
MANY_LAG_RANGE_TEST = os.path.join(LIBDIR, "muse_many_lag_range_test")
ROWS_LAG_RANGE_TEST = os.path.join(LIBDIR, "muse_rows_lag_range_test")
SIGNED_LAG_RANGE_TEST = os.path.join(LIBDIR, "muse_signed_lag_range_test")
LAG_BAND_TEST = os.path.join(LIBDIR, "muse_lag_band_test")
MANY_LAG_BAND_TEST = os.path.join(LIBDIR, "muse_many_lag_band_test")
LAG_PROFILE_TEST = os.path.join(LIBDIR, "muse_lag_profile_test")


def build_host_test(force=False):
    """The C++ host mirror's test program."""
    return _build_host_program("muse_host_test", "-O1", force)


def build_ref_bench(force=False):
    """The reference's own benchmark shapes over the host mirror (bench.py runs it)."""
    return _build_host_program("muse_ref_bench", "-O2", force)


def build_cold_phases(force=False):
    """The cold-path phase breakdown (profiles/r06_cold_path.txt)."""
    return _build_host_program("muse_cold_phases", "-O2", force)


def build_resident_test(force=False):
    """The host mirror's resident-row reuse test (tests/test_gpu_resident_rows.py)."""
    return _build_host_program("muse_resident_test", "-O1", force)


def build_window_test(force=False):
    """The host mirror's lag-window program (tests/test_gpu_lag_window.py)."""
    return _build_host_program("muse_window_test", "-O1", force)


def build_window_many_test(force=False):
    """The host mirror's windowed many-references program (tests/test_gpu_lag_window_many.py)."""
    return _build_host_program("muse_window_many_test", "-O1", force)


def build_rows_window_test(force=False):
    """The host mirror's windowed Muse.Run program (tests/test_gpu_window_rows.py)."""
    return _build_host_program("muse_rows_window_test", "-O1", force)


def build_in_window_test(force=False):
    """The host mirror's wide-window program (tests/test_gpu_in_window.py)."""
    return _build_host_program("muse_in_window_test", "-O1", force)


def build_lag_range_test(force=False):
    """The host mirror's one-sided / asymmetric window program (tests/test_gpu_lag_range.py)."""
    return _build_host_program("muse_lag_range_test", "-O1", force)


def build_many_in_window_test(force=False):
    """The host mirror's wide-window many-references program (tests/test_gpu_many_in_window.py)."""
    return _build_host_program("muse_many_in_window_test", "-O1", force)


def build_many_lag_range_test(force=False):
    """The host mirror's many-references lag-range program (tests/test_gpu_many_lag_range.py)."""
    return _build_host_program("muse_many_lag_range_test", "-O1", force)


def build_rows_lag_range_test(force=False):
    """The host mirror's Muse.Run lag-range program (tests/test_gpu_rows_lag_range.py)."""
    return _build_host_program("muse_rows_lag_range_test", "-O1", force)


def build_signed_lag_range_test(force=False):
    """The host mirror's signed lag-range program (tests/test_gpu_signed_lag_range.py)."""
    return _build_host_program("muse_signed_lag_range_test", "-O1", force)


def build_lag_band_test(force=False):
    """The host mirror's lag-band program (tests/test_gpu_lag_band.py)."""
    return _build_host_program("muse_lag_band_test", "-O1", force)


def build_many_lag_band_test(force=False):
    """The host mirror's many-references lag-band program (tests/test_gpu_many_lag_band.py)."""
    return _build_host_program("muse_many_lag_band_test", "-O1", force)


def build_lag_profile_test(force=False):
    """The host mirror's lag-profile program (tests/test_gpu_lag_profile.py)."""
    return _build_host_program("muse_lag_profile_test", "-O1", force)
