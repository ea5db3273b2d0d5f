"""GPU sweep of the lag-window kernels over every lag of every window (run with -m gpu on an MI355X): xcorr_window_mfma through
DeviceBatch.set_lag_window, the split-K kernels through the windowed Muse.Run's per-row hook, the packed many-references pass and
the fused slide-and-score kernel.

The other windowed GPU files compare with the FFT oracle at 1e-6 relative on a broad rectangular pulse and at 11 of the 64 windows.
Here every row is constructed to win at a CHOSEN lag (tests/_winsweep.py: one row per lag in [-63, 63], rows just outside whose
best match inside a window is a sidelobe, rows with a far-outlier first sample), every window L = 0 .. 63 is scored, and every test
asserts three things against the long-double table of the definition (no oracle call, no FFT):

  * the NaN pattern is empty;
  * the lag is exact on every row -- tests/test_window_sweep_cpu.py shows that the construction leaves every row's two largest
    |cc| inside every window at least 100 (B_first + B_second) apart (asserted again here before anything is compared);
  * |mv - cc_ld| <= B, the derived rounding bound of tests/_winsweep.py (no fitted constant): 7e-16 ... 1.4e-12 on ordinary rows
    (7e-12 at N = 35841), up to 1.1e-9 on the rows whose first sample lies 50 sigma off (1.3e-8 at N = 35841).  Measured on one
    MI355X: at most 5.9e-15 on ordinary rows and 8.9e-13 on the outlier rows, 0.076 of B at the worst (N = 64).

The measured worst error and worst err / B of every case are printed before anything is asserted, the outlier rows' separately;
MUSE_TEST_WORST=<file> appends them (profiles/window_sweep_parity.txt is such a run)."""
import os

import numpy as np
import pytest

import _winsweep as WS
from _load import pkg

pytestmark = pytest.mark.gpu

ALL_LS = tuple(range(WS.LMAX + 1))
SUBSET_ROWS = (1, 15, 16, 17)     # a lone row, a partial block, a block boundary, a block and one row
SUBSET_LS = (0, 7, 8, 63)


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
    e = muse.Engine(0)                       # a context of its own: the hooks set below never leak into other test files
    yield e
    e.close()


# ------------------------------------------------------------------ cases and expectations: computed once, never changed
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _with_tables(case):
    return case, [WS.tables(ref, case.rows, case.n) for ref in case.refs]


def single(N):
    return _cached(("single", N), lambda: _with_tables(WS.sweep_case(N)))


def want(table, L):
    """(lag, mv, B) of window L from a table; the gap condition is asserted here, before anything is compared with it"""
    if not hasattr(table, "want"):
        table.want = {}
    if L not in table.want:
        lag, mv, B, ratio = WS.expect(table, L)
        assert float(ratio.min()) >= WS.GAP_FACTOR, (L, float(ratio.min()))
        table.want[L] = (lag, mv, B)
    return table.want[L]


class Sweep:
    """collects the comparisons of one case over its windows; report() prints and records the worst figures, then asserts"""

    def __init__(self, tag):
        self.tag, self.calls, self.rows = tag, 0, 0
        self.worst, self.ratio, self.far_rows, self.far_worst, self.far_ratio = 0.0, 0.0, 0, 0.0, 0.0
        self.b, self.far_b = [np.inf, 0.0], [np.inf, 0.0]        # smallest and largest B compared against
        self.nan, self.lags, self.over = [], [], []

    def add(self, what, got, expected, outlier, first=None):
        """got: (lag, mv) of the kernel; expected: want(); first: compare the first `first` rows only"""
        lag, mv = np.asarray(got[0]), np.asarray(got[1], dtype=np.float64)
        elag, emv, B = (a if first is None else a[:first] for a in expected)
        outlier = outlier if first is None else outlier[:first]
        assert lag.shape == mv.shape == elag.shape == B.shape, (self.tag, what, lag.shape, elag.shape)
        err = np.abs(mv.astype(np.longdouble) - emv).astype(np.float64)
        err[~np.isfinite(err)] = np.inf
        rel = err / B
        self.calls += 1
        self.rows += len(lag)
        if (~outlier).any():
            self.worst, self.ratio = max(self.worst, float(err[~outlier].max())), max(self.ratio, float(rel[~outlier].max()))
            self.b = [min(self.b[0], float(B[~outlier].min())), max(self.b[1], float(B[~outlier].max()))]
        if outlier.any():
            self.far_rows = int(outlier.sum())
            self.far_worst, self.far_ratio = max(self.far_worst, float(err[outlier].max())), max(self.far_ratio, float(rel[outlier].max()))
            self.far_b = [min(self.far_b[0], float(B[outlier].min())), max(self.far_b[1], float(B[outlier].max()))]
        if np.isnan(mv).any():
            self.nan.append((what, np.nonzero(np.isnan(mv))[0][:4].tolist()))
        bad = np.nonzero(lag != elag)[0]
        if bad.size:
            self.lags.append((what, bad[:4].tolist(), lag[bad[:4]].tolist(), elag[bad[:4]].tolist()))
        over = np.nonzero(err > B)[0]
        if over.size:
            self.over.append((what, over[:4].tolist(), err[over[:4]].tolist(), B[over[:4]].tolist()))

    def report(self):
        line = "%s: %d passes, %d scores, worst=%.3e, worst err/B=%.4f, B=%.1e..%.1e" % (
            self.tag, self.calls, self.rows, self.worst, self.ratio, self.b[0], self.b[1])
        if self.far_rows:
            line += " | %d rows with a far first sample: worst=%.3e, worst err/B=%.4f, B=%.1e..%.1e" % (
                self.far_rows, self.far_worst, self.far_ratio, self.far_b[0], self.far_b[1])
        print(line)
        path = os.environ.get("MUSE_TEST_WORST")
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")
        assert self.calls > 0
        assert not self.nan, "%s: NaN scores (pass, rows): %s" % (self.tag, self.nan[:4])
        assert not self.lags, "%s: lags off the table's (pass, rows, got, expected): %s" % (self.tag, self.lags[:4])
        assert not self.over, "%s: scores outside B (pass, rows, errors, bounds): %s" % (self.tag, self.over[:4])


def build_name(n, N, L):
    """the instantiation launch_window picks: accumulator tiles of 16 lags for the clipped window, WIDE iff the rows are 16-byte aligned"""
    Lc = min(L, n // 2)
    return "xcorr_window_mfma<%d, %s>" % ((2 * Lc + 16) // 16, "true" if N % 2 == 0 else "false")


# ------------------------------------------------------------------ a. xcorr_window_mfma, every L
@pytest.mark.parametrize("N", WS.LENGTHS)
def test_window_every_lag(muse, eng, N):
    """DeviceBatch.set_lag_window(L) + scores() for L = 0 .. 63 on the full row set (12 full 16-row blocks and a partial one from
    N = 480 on), then on the first 1, 15, 16 and 17 rows at the windows either side of the one-tile | two-tile cut and at the ends;
    the kernel's name must report the build that (2 L + 16) // 16 tiles and the rows' alignment predict"""
    case, (table,) = single(N)
    sw = Sweep("xcorr_window_mfma N=%d n=%d rows=%d" % (N, case.n, len(case.rows)))
    builds = set()
    for M in (len(case.rows),) + SUBSET_ROWS:
        dg = muse.DeviceGroup.from_rows(eng, case.rows[:M])
        db = muse.DeviceBatch(eng, dg, case.ref)
        try:
            assert db.n == case.n
            for L in (ALL_LS if M == len(case.rows) else SUBSET_LS):
                db.set_lag_window(L)
                name = eng.kernel_name(db)
                assert name == build_name(case.n, N, L), (N, L, name)
                builds.add(name)
                sw.add("M=%d L=%d" % (M, L), db.scores(), want(table, L), case.outlier, first=M)
        finally:
            db.close()
            dg.close()
    sw.report()
    assert len(builds) == (8 if case.n >= 128 else (2 * (case.n // 2) + 16) // 16)      # every TILES build the length reaches


# ------------------------------------------------------------------ b. split-K
class forced:
    """the windowed Muse.Run of `eng` in S slices for the length of a with-block (0 = the planner)"""

    def __init__(self, eng, S, always_copy=False):
        self.eng, self.S, self.copy = eng, S, always_copy

    def __enter__(self):
        self.eng.window_rows_slices(self.S)
        self.eng.rows_always_copy(self.copy)

    def __exit__(self, *a):
        self.eng.window_rows_slices(0)
        self.eng.rows_always_copy(False)


def _split_sweep(muse, eng, case, table, slices):
    N = case.N
    chunks = (N + 1023) // 1024
    probe = muse.DeviceGroup(eng, N, 0)
    tmpl = muse.DeviceBatch(eng, probe, case.ref)
    try:
        assert tmpl.n == case.n
        for S in slices:
            assert S <= chunks                                   # (the hook clips S to the chunk count: every S here is taken as it is)
            sw = Sweep("split-K N=%d S=%s rows=%d" % (N, S if S else "planner", len(case.rows)))
            for L in ALL_LS:
                with forced(eng, S):
                    got = tmpl.run_rows_windowed_scores(case.rows, L)
                sw.add("L=%d" % L, got, want(table, L), case.outlier)
            sw.report()
        sw = Sweep("split-K N=%d S=%d L=15 rows copied / read in place" % (N, slices[0]))
        for always_copy in (True, False):
            with forced(eng, slices[0], always_copy):
                got = tmpl.run_rows_windowed_scores(case.rows, 15)
            sw.add("copy=%s" % always_copy, got, want(table, 15), case.outlier)
        sw.report()
        assert tmpl.lag_window() == -1
    finally:
        eng.window_rows_slices(0)
        eng.rows_always_copy(False)
        tmpl.close()
        probe.close()


@pytest.mark.parametrize("N,slices", [(2049, (2, 3)), (5000, (2, 3, 5))])
def test_split_every_lag(muse, eng, N, slices):
    """tmpl.run_rows_windowed_scores under a forced slice count: N = 2049 is 3 chunks, the last one sample long, odd stride;
    N = 5000 is 5 chunks with N < n"""
    case, (table,) = single(N)
    _split_sweep(muse, eng, case, table, slices)


def test_split_every_lag_long_rows(muse, eng):
    """N = 35841 -- 35 chunks plus one sample -- with 17 rows at lags spread over [-63, 63] and their outlier copies: 2 slices, 16
    (the last count with single-chunk slices allowed), 17 (the first in the 'at least two chunks per slice' regime: uneven slices
    of 2 and 3 chunks) and the planner's own choice"""
    case, (table,) = _cached(("long",), lambda: _with_tables(WS.long_case()))
    S, cps = muse.window_rows_plan(len(case.rows), case.N, 256)
    assert S > 1                                                 # (whatever the device's CU count: few rows of long series are split)
    _split_sweep(muse, eng, case, table, (2, 16, 17, 0))


# ------------------------------------------------------------------ c. many references
def expected_launches(R, L):
    """references of window L are packed while R (2 L + 1) <= 128 rows fit one product; from L = 24 on (more than
    WINM_PACK_MAX_ROWS = 48 rows each) they are not packed: one launch per reference"""
    W = 2 * L + 1
    if W > 48:
        return R
    per = 128 // W
    return (R + per - 1) // per


@pytest.mark.parametrize("N", WS.MANY_LENGTHS)
def test_many_references_every_lag(muse, eng, N):
    """muse.scores_many_windowed over R = 3 and R = 8 references that carry the code at p + offset: reference i's winner for a row
    is the row's lag shifted by the offset, so one row set sweeps every reference's window at other rows; each batch is checked
    against its own table, the planner's launch count on the host"""
    case, tabs = _cached(("many", N), lambda: _with_tables(WS.many_case(N)))
    dg = muse.DeviceGroup.from_rows(eng, case.rows)
    dbs = [muse.DeviceBatch(eng, dg, ref) for ref in case.refs]
    try:
        for R in (3, 8):
            sws = [Sweep("many-references N=%d R=%d reference %d (offset %+d)" % (N, R, i, case.offsets[i])) for i in range(R)]
            for L in ALL_LS:
                plan = muse.window_many_plan(R, L)
                assert plan["launches"] == expected_launches(R, L), (R, L, plan["launches"])
                assert (plan["launches"] == 1) == (R * (2 * L + 1) <= 128)
                got = muse.scores_many_windowed(dbs[:R], L)
                for i in range(R):
                    sws[i].add("L=%d" % L, got[i], want(tabs[i], L), case.outlier)
                    assert dbs[i].lag_window() == -1
            for sw in sws:
                sw.report()
    finally:
        for db in dbs:
            db.close()
        dg.close()


# ------------------------------------------------------------------ d. slide and score
@pytest.mark.parametrize("N", WS.SLIDE_LENGTHS)
@pytest.mark.parametrize("k", WS.SLIDE_KS)
def test_slide_score_every_call(muse, eng, N, k):
    """DeviceBatch.slide_score_windowed(tails, L), four calls in a row from the case's rows: after each the group reads back the
    host-rolled rows bit for bit, and the scores match the table recomputed on those rows -- the planted lag walks by k per
    call, through the window and out of it.  k = 1: 8-byte loads; 16 and 64: 16-byte loads at even N"""
    case, _ = single(N)

    def states():
        image = WS.Image(case.ref, case.n)
        return [(tails, rows, WS.tables(case.ref, rows, case.n, image)) for tails, rows in WS.slide_states(case, k)]
    st = _cached(("slide", N, k), states)
    none = np.zeros(len(case.rows), dtype=bool)          # (the outlier sample has left the row with the first slide)
    sw = Sweep("slide-and-score N=%d k=%d" % (N, k))
    for L in WS.SLIDE_LS:
        dg = muse.DeviceGroup.from_rows(eng, case.rows)
        db = muse.DeviceBatch(eng, dg, case.ref)
        try:
            for call, (tails, rows, table) in enumerate(st, 1):
                db.slide_score_windowed(tails, L)
                got = db.read_scores()
                held = dg.read(0, len(rows))
                assert held.tobytes() == rows.tobytes(), (N, k, L, call)
                sw.add("L=%d call %d" % (L, call), got, want(table, L), none)
            assert dg.slides == len(st) and db.lag_window() == -1
        finally:
            db.close()
            dg.close()
    sw.report()
