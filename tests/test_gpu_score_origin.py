"""GPU test of the record of where a batch's scores came from (muse_batch::origin, capi_internal.h; run with -m gpu on an MI355X).

One batch walks a fixed table of scoring passes, selections and refused calls; after every step muse_batch_kernel_name and
muse_test_last_in_window_path must report the pass that filled mv / lag.  That pins the record's two rules: every pass overwrites
it as a whole (nothing of the pass before shows through: a window, a tile count, the many-references marker), and a selection
or a refused call leaves it alone.  The names are the ones the tests of each pass expect (test_gpu_in_window.py,
test_gpu_many_in_window.py, test_gpu_lag_window_many.py, test_gpu_lag_sweep.py), here in full; the scores themselves are those
tests' business."""
import numpy as np
import pytest

import _window as W
from _load import pkg

pytestmark = pytest.mark.gpu

NARROW, WIDE = 8, 100          # a window the direct product takes on float64 rows; one beyond MUSE_LAG_WINDOW_MAX (the masked kernels)


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return m


@pytest.fixture(scope="module")
def eng(muse):
    return muse.get_engine(0)


class _Names:
    """the instantiations muse_batch_kernel_name reports for series of N samples (capi_batch.hip)"""

    def __init__(self, N, f32):
        self.n = 1 << (N - 1).bit_length()
        self.logn = self.n.bit_length() - 1
        self.padded = "true" if N < self.n else "false"
        self.f32 = "true" if f32 else "false"

    def own(self, win=""):          # automatic selection on a small group: the default kernel of the length
        if self.n == 4096:
            return "xcorr_fused_n4096_fold<false, %s, %s%s>" % (self.padded, self.f32, win)
        return "xcorr_fused_small<%d, %s, false, %s%s>" % (self.logn, self.padded, self.f32, win)

    def masked(self):               # the same kernel's WIN build
        return self.own(", true")

    def masked_many(self):          # the one masked many-references pass
        if self.n == 4096:
            return "xcorr_fused_n4096_fold_multi<%s, %s, true>" % (self.padded, self.f32)
        return "xcorr_fused_small<%d, %s, true, false, true>" % (self.logn, self.padded)

    @staticmethod
    def mfma(L):                    # the direct product: its accumulator tiles, then the row layout
        return "xcorr_window_mfma<%d, " % ((2 * L + 1 + 15) // 16)


@pytest.mark.parametrize("M,N,f32", [(96, 600, False), (64, 4096, False), (64, 4096, True)])
def test_every_pass_names_itself(muse, eng, M, N, f32):
    B = muse.binding
    ref, rows = W.make_case(N, M, seed=N + M)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    b = muse.DeviceBatch(eng, dg, ref)
    b2 = muse.DeviceBatch(eng, dg, np.roll(ref, 5))
    nm = _Names(N, f32)
    assert b.n == nm.n
    plan = muse.window_many_plan(2, NARROW)
    assert plan["launches"] == 1                     # both references' windows in one packed launch
    packed = "xcorr_window_many_mfma<%d, " % int(plan["tiles_of"][0])
    no_tails = np.zeros((M, 0))

    def state():
        return eng.kernel_name(b), b.last_in_window_path()

    def step(tag, call, name, path, exact=True):
        call()
        got = state()
        assert got[1] == path and (got[0] == name if exact else got[0].startswith(name)), (tag, got, name, path)

    def refused(tag, call, status=B.MUSE_ERR_UNSUPPORTED):
        before = state()
        with pytest.raises(muse.MuseError) as e:
            call()
        assert e.value.status == status, (tag, e.value)
        assert state() == before, (tag, state(), before)

    step("1 score", b.score, nm.own(), 0)
    if f32:                                          # float32 storage has no direct product: the masked kernel at any width
        step("2 score_in_window", lambda: b.score_in_window(NARROW), nm.masked(), B.MUSE_IN_WINDOW_MASKED)
    else:
        step("2 score_in_window", lambda: b.score_in_window(NARROW), nm.mfma(NARROW), B.MUSE_IN_WINDOW_MFMA, exact=False)
    step("3 run", lambda: b.run(None, 0, max_lag=10, top_n=5), nm.own(), 0)
    if f32:
        refused("4 scores_many_windowed", lambda: muse.scores_many_windowed([b, b2], NARROW))
    else:
        step("4 scores_many_windowed", lambda: muse.scores_many_windowed([b, b2], NARROW), packed, 0, exact=False)
    step("5 run_many_in_window", lambda: muse.run_many_in_window([b, b2], max_lag=WIDE, top_n=5), nm.masked_many(),
         B.MUSE_IN_WINDOW_MASKED)
    assert state() == (eng.kernel_name(b2), b2.last_in_window_path())
    step("6 score_many", lambda: muse.score_many([b, b2]), nm.own(), 0)
    if f32:
        refused("7 set_lag_window", lambda: b.set_lag_window(NARROW))
    else:
        b.set_lag_window(NARROW)
        step("7 set_lag_window + score", b.score, nm.mfma(NARROW), 0, exact=False)
        step("7 window off", lambda: b.set_lag_window(-1), nm.own(), 0)   # (the own setting again: what the next score takes)
    step("8 run_in_window", lambda: b.run_in_window(WIDE, top_n=5), nm.masked(), B.MUSE_IN_WINDOW_MASKED)
    if f32:
        refused("9 slide_score_windowed", lambda: b.slide_score_windowed(no_tails, NARROW))
    else:   # (its window is the call's, its record the batch's own setting: with the window off that names the default kernel)
        step("9 slide_score_windowed", lambda: b.slide_score_windowed(no_tails, NARROW), nm.own(), 0)
    # refused for every storage: a bad window, a bad selection argument in front of a pass, a list with the same batch twice
    b.score_in_window(WIDE)
    assert state() == (nm.masked(), B.MUSE_IN_WINDOW_MASKED)
    refused("score_in_window(-1)", lambda: b.score_in_window(-1), B.MUSE_ERR_INVALID)
    refused("run_in_window, bad sign_filter", lambda: b.run_in_window(NARROW, top_n=5, sign_filter=2), B.MUSE_ERR_INVALID)
    refused("score_many_in_window, batch twice", lambda: muse.score_many_in_window([b, b], WIDE), B.MUSE_ERR_INVALID)
    step("10 score", b.score, nm.own(), 0)
    for h in (b, b2, dg):
        h.close()
