"""GPU sweep of the lag-RANGE kernels over every lag of every range (run with -m gpu on an MI355X): the direct product from any
table origin, unsigned and signed (xcorr_window_mfma / xcorr_window_signed_mfma); the panel kernels of Muse.Run inside 128 .. 2048
lags (xcorr_window_panel_partial / window_panels_finish); the masked argmax of the transform kernels, unsigned and signed
(mask_window, mask_window_quot); the many-references forms.

The other range files compare with the FFT oracle at 1e-6 relative on rows whose winners sit wherever a random shift put them.  Here
every row is constructed to win at a CHOSEN lag (tests/_rangesweep.py), every range of a list that reaches every tile count, every
origin residue, every panel boundary and every mask register is scored under sign 0, +1 and -1 (the signed passes on `rows` and on
`-rows`, so that each planted lag wins under both signs), and every pass is held to

  * an empty NaN pattern and the kernel the dispatch table names;
  * the lag, exact on EVERY row: tests/test_range_sweep_cpu.py shows that the two largest keys inside every range lie at least
    100 (B_first + B_second) apart, asserted again here before anything is compared;
  * |mv - cc_ld| <= B on the direct product and the panels: the long-double table and the derived rounding bound of
    tests/_winsweep.py (no fitted constant).  On the masked transform passes a row planted inside the range, and of the sign, is
    held to its planted lag and to _lagsweep.ld_score_at within _lagsweep.row_bounds; every other row -- whose 0.9 peak lies just
    outside a bound or has the other sign, so that a leaking mask would report it -- to the definition on the oracle's correlation
    at 1e-6 / 1e-12 with the lag exact, no tie allowed, and lag != planted.

The gap condition leaves the panels' tie-break idle, so exact ties have a test of their own
(test_panels_exact_ties_take_the_first_in_scan_order).

The measured worst error and worst err / B of every case are printed before anything is asserted; MUSE_TEST_WORST=<file> appends
them (profiles/range_sweep_parity.txt is such a run).  Measured on one MI355X: direct product at most 5.5e-15 off the table, 0.073
of B at N = 64 and at most 0.013 from N = 480 on; panels 2.9e-15, 0.0076 of B; rows with a far first sample 1.9e-13, at most 0.013
of their B; masked passes within 0.042 of row_bounds on planted rows and 2e-11 relative on the others."""
import os

import numpy as np
import pytest

import _lagrange as LR
import _lagsweep as LS
import _rangesweep as RS
import _rowslagrange as RL
import _winsweep as WS
from _load import pkg
from test_gpu_window_sweep import Sweep

pytestmark = pytest.mark.gpu


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


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def want(table, lo, hi, sign):
    """(lag, mv, B) of the range under the sign; the gap condition is asserted here, before anything is compared with it"""
    if not hasattr(table, "want"):
        table.want = {}
    key = (lo, hi, sign)
    if key not in table.want:
        lag, mv, B, ratio = RS.expect(table, lo, hi, sign)
        assert float(ratio.min()) >= RS.GAP_FACTOR, (key, float(ratio.min()))
        table.want[key] = (lag, mv, B)
    return table.want[key]


def no_sign_bit(got, expected, sign, tag):
    """under a sign, a series with nothing of the sign is exactly (0, +0.0): the sign bit clear"""
    if sign:
        none = np.asarray(expected[1] == 0)
        assert np.all(got[0][none] == 0) and np.all(got[1][none] == 0.0) and not np.signbit(got[1][none]).any(), tag
        return int(none.sum())
    return 0


def groups_of(case, table):
    """(name, rows, table, signs): sign 0 and both signs on the rows, both signs on the negated rows"""
    return (("rows", case.rows, table, RS.SIGNS), ("-rows", -case.rows, RS.negated(table), (1, -1)))


# ------------------------------------------------------------------ a. the direct product from any origin
def direct_name(n, N, lo, hi, sign):
    wide = "true" if N % 2 == 0 else "false"
    if sign:
        return "xcorr_window_signed_mfma<%d, %s, %d>" % (RS.tiles_of(n, lo, hi), wide, sign)
    return "xcorr_window_mfma<%d, %s>" % (RS.tiles_of(n, lo, hi), wide)


@pytest.mark.parametrize("N", RS.DIRECT_LENGTHS)
def test_direct_product_every_lag_of_every_range(muse, eng, N):
    """scores_in_lag_range / scores_signed_in_lag_range over every one-sided range, the widest range at every origin and 200
    random ranges: every table row and accumulator-tile element wins somewhere, and the unwrap of the scan position is taken at
    every origin"""
    B = muse.binding
    case = _cached(("direct", N), lambda: RS.direct_case(N))
    table = _cached(("direct-table", N), lambda: WS.tables(case.ref, case.rows, case.n, lags=RS.direct_table_lags(case.n)))
    ranges = RS.direct_ranges(N)
    tiles, residues, none = set(), set(), 0
    for gname, rows, tab, signs in groups_of(case, table):
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, case.ref)
        try:
            assert db.n == case.n
            for s in signs:
                sw = Sweep("direct product N=%d n=%d %s sign %+d rows=%d" % (N, case.n, gname, s, len(rows)))
                for lo, hi in ranges:
                    if RS.every_lag(case.n, lo, hi):
                        # N = n = 64 alone: clipped, the range is every lag, which is not the direct product's -- without a sign the
                        # plain pass (held to the lag, and to the transform kernels' bound on top of B), with one not built
                        assert N == 64
                        if s:
                            with pytest.raises(muse.MuseError) as e:
                                db.score_signed_in_lag_range(lo, hi, s)
                            assert e.value.status == B.MUSE_ERR_UNSUPPORTED
                        else:
                            lag, mv = db.scores_in_lag_range(lo, hi)
                            elag, emv, eB = want(tab, lo, hi, 0)
                            assert db.last_in_window_path() == B.MUSE_IN_WINDOW_PLAIN and np.array_equal(lag, elag)
                            assert np.all(np.abs(mv.astype(np.longdouble) - emv) <= eB + LS.bound(case.n)), (lo, hi)
                        continue
                    got = db.scores_signed_in_lag_range(lo, hi, s) if s else db.scores_in_lag_range(lo, hi)
                    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA, (N, lo, hi, s, db.last_in_window_path())
                    name = eng.kernel_name(db)
                    assert name == direct_name(case.n, N, lo, hi, s), (N, lo, hi, s, name)
                    exp = want(tab, lo, hi, s)
                    sw.add("[%d, %d]" % (lo, hi), got, exp, case.outlier)
                    none += no_sign_bit(got, exp, s, (N, gname, lo, hi, s))
                    tiles.add(RS.tiles_of(case.n, lo, hi))
                    residues.add(-LR.clip(case.n, lo, hi)[0] % 16)
                sw.report()
        finally:
            db.close()
            dg.close()
    assert tiles == set(range(1, (8 if case.n >= 256 else RS.tiles_of(case.n, -RS.RMAX, RS.RMAX)) + 1))
    assert residues == set(range(16))
    assert none > 0


# ------------------------------------------------------------------ b. the panel kernels
class forced:
    """the slice count of the windowed Muse.Run of `eng` for the length of a with-block (0 = the planner)"""

    def __init__(self, eng, S):
        self.eng, self.S = eng, S

    def __enter__(self):
        self.eng.window_rows_slices(self.S)

    def __exit__(self, *a):
        self.eng.window_rows_slices(0)


def _panel_sweep(muse, eng, tag, case, table, ranges, slices):
    """run_rows_in_lag_range_scores over `ranges` at every slice count; at S = 1 the rows that win inside a sub-range of at most
    127 lags carry the bits of the batch's own direct product on that sub-range"""
    N, M = case.N, len(case.rows)
    cus = eng.device_info()[1]
    probe = muse.DeviceGroup(eng, N, 0)
    tmpl = muse.DeviceBatch(eng, probe, case.ref)
    dg = muse.DeviceGroup.from_rows(eng, case.rows)
    db = muse.DeviceBatch(eng, dg, case.ref)
    try:
        assert tmpl.n == case.n
        sws = {S: Sweep("panels %s N=%d S=%s rows=%d" % (tag, N, S if S else "planner", M)) for S in slices}
        sub = Sweep("panels %s N=%d: the direct product on the sub-ranges" % (tag, N))
        same = 0
        for lo, hi in ranges:
            path, panels, S0 = muse.rows_lag_range_plan(M, N, cus, lo, hi)
            assert path == RL.PANELS and panels == -(-(hi - lo + 1) // RS.PANEL), (lo, hi, path, panels)
            exp = want(table, lo, hi, 0)
            for S in slices:
                with forced(eng, S):
                    got = tmpl.run_rows_in_lag_range_scores(case.rows, lo, hi)
                sws[S].add("[%d, %d]" % (lo, hi), got, exp, case.outlier)
                if S != 1:
                    continue
                for a, b in RS.sub_ranges(lo, hi):
                    narrow = db.scores_in_lag_range(a, b)
                    sub.add("[%d, %d] of [%d, %d]" % (a, b, lo, hi), narrow, want(table, a, b, 0), case.outlier)
                    ins = (exp[0] >= a) & (exp[0] <= b)
                    assert np.array_equal(got[0][ins], narrow[0][ins]) and got[1][ins].tobytes() == narrow[1][ins].tobytes(), (N, lo, hi, a, b)
                    same += int(ins.sum())
        for S in slices:
            sws[S].report()
        sub.report()
        assert same > 0 and tmpl.lag_window() == -1
    finally:
        eng.window_rows_slices(0)
        for h in (db, dg, tmpl, probe):
            h.close()


@pytest.mark.parametrize("N", RS.PANEL_LENGTHS)
def test_panels_every_lag_of_few_panels(muse, eng, N):
    """one row per lag in [-180, 180]; 128 .. 361 lags from three origins each: two and three panels, a last panel of one row
    ((-128, 0), (0, 128)), of 127 and of a full 128 rows; the planner's slice count and 1, 2, 3 forced"""
    case = _cached(("panel", N), lambda: RS.panel_case(N))
    table = _cached(("panel-table", N), lambda: WS.tables(case.ref, case.rows, case.n, lags=RS.panel_table_lags()))
    _panel_sweep(muse, eng, "few", case, table, RS.panel_ranges(), RS.PANEL_SLICES)


@pytest.mark.parametrize("which", [c[0] for c in RS.SIXTEEN])
def test_sixteen_panels(muse, eng, which):
    """2048 lags: winners at table rows 128 z + {-2, -1, 0, 1} of every panel, at both ends and just outside either end"""
    case, (lo, hi) = _cached(("sixteen", which), lambda: RS.sixteen_case(which))
    table = _cached(("sixteen-table", which), lambda: WS.tables(case.ref, case.rows, case.n, lags=np.arange(lo, hi + 1)))
    assert muse.rows_lag_range_plan(len(case.rows), case.N, eng.device_info()[1], lo, hi)[1] == 16
    _panel_sweep(muse, eng, which, case, table, ((lo, hi),), RS.SIXTEEN_SLICES)


def test_panels_exact_ties_take_the_first_in_scan_order(muse, eng):
    """rows whose largest |cc| stands at several lags with the same bits (tests/_rangesweep.py: a reference of exact period 30, rows
    of two opposite impulses): the panels arrive in table order and must still report the FIRST of the tied lags in the
    definition's scan order -- the `pos` total order of the finish kernel, which the gap condition of every other case leaves idle"""
    ref, rows = _cached(("ties",), RS.tie_case)
    n = LS.fft_len(RS.TIE_N)
    table = _cached(("ties-table",), lambda: WS.tables(ref, rows, n, lags=RS.tie_table_lags()))
    probe = muse.DeviceGroup(eng, RS.TIE_N, 0)
    tmpl = muse.DeviceBatch(eng, probe, ref)
    none = np.zeros(len(rows), dtype=bool)
    try:
        sw = Sweep("panels, exact ties N=%d rows=%d" % (RS.TIE_N, len(rows)))
        for lo, hi in RS.TIE_RANGES:
            lag, mv, B, ratio, ties = RS.expect_tied(table, lo, hi)
            assert ties.min() >= 2 and float(ratio.min()) >= RS.GAP_FACTOR, (lo, hi)
            assert muse.rows_lag_range_plan(len(rows), RS.TIE_N, eng.device_info()[1], lo, hi)[0] == RL.PANELS
            for S in RS.TIE_SLICES:
                with forced(eng, S):
                    got = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
                sw.add("[%d, %d] S=%d" % (lo, hi, S), got, (lag, mv, B), none)
        sw.report()
    finally:
        eng.window_rows_slices(0)
        tmpl.close()
        probe.close()


# ------------------------------------------------------------------ c. the masked transform kernels
class Masked:
    """collects the two-tier comparison of one masked case over its ranges, signs and row groups; report() prints and records the
    worst figures, then asserts"""

    def __init__(self, tag):
        self.tag, self.calls, self.rows1, self.rows2 = tag, 0, 0, 0
        self.worst1, self.ratio1, self.rel2, self.bad = 0.0, 0.0, 0.0, []

    def add(self, what, got, m, lo, hi, sign, g):
        lag, mv = np.asarray(got[0]), np.asarray(got[1], dtype=np.float64)
        tier1, elag, emv, tie = RS.masked_want(m, lo, hi, sign, g)
        self.calls += 1
        if np.isnan(mv).any():
            self.bad.append((what, "NaN", np.nonzero(np.isnan(mv))[0][:4].tolist()))
            return
        clo, chi = LR.clip(m.n, lo, hi)
        if not np.all((lag >= clo) & (lag <= chi)):
            self.bad.append((what, "lag outside the range", np.nonzero((lag < clo) | (lag > chi))[0][:4].tolist()))
        if sign and not np.all(sign * mv >= 0):
            self.bad.append((what, "value of the other sign", np.nonzero(sign * mv < 0)[0][:4].tolist()))
        # tier 1: planted inside the range and of the sign
        t1 = np.nonzero(tier1)[0]
        self.rows1 += len(t1)
        if len(t1):
            err = np.abs(mv[t1].astype(np.longdouble) - g * m.ld[t1]).astype(np.float64)
            self.worst1, self.ratio1 = max(self.worst1, float(err.max())), max(self.ratio1, float((err / m.bounds[t1]).max()))
            off = t1[lag[t1] != m.pl[t1]]
            if off.size:
                self.bad.append((what, "planted lag lost", off[:4].tolist(), lag[off[:4]].tolist(), m.pl[off[:4]].tolist()))
            over = t1[err > m.bounds[t1]]
            if over.size:
                self.bad.append((what, "score outside the bound", over[:4].tolist()))
        # tier 2: everything else, against the definition on the oracle's correlation
        t2 = np.nonzero(~tier1)[0]
        self.rows2 += len(t2)
        if len(t2):
            if tie[t2].any():
                self.bad.append((what, "the oracle flags a tie", t2[tie[t2]][:4].tolist()))
            err = np.abs(mv[t2] - emv[t2])
            nz = np.abs(emv[t2]) > 0
            if nz.any():
                self.rel2 = max(self.rel2, float((err[nz] / np.abs(emv[t2][nz])).max()))
            over = t2[err > RS.SCORE_RTOL * np.abs(emv[t2]) + RS.SCORE_ATOL]
            if over.size:
                self.bad.append((what, "score off the oracle's", over[:4].tolist()))
            off = t2[lag[t2] != elag[t2]]
            if off.size:
                self.bad.append((what, "lag off the oracle's", off[:4].tolist(), lag[off[:4]].tolist(), elag[off[:4]].tolist()))
            none = (emv[t2] == 0) if sign else np.zeros(len(t2), dtype=bool)   # (nothing of the sign: lag 0 whatever was planted)
            leak = t2[(lag[t2] == m.pl[t2]) & ~none]
            if leak.size:
                self.bad.append((what, "the planted lag reported through the mask", leak[:4].tolist()))
            if sign:
                z = t2[emv[t2] == 0]
                if not (np.all(lag[z] == 0) and np.all(mv[z] == 0.0) and not np.signbit(mv[z]).any()):
                    self.bad.append((what, "nothing of the sign is not (0, +0.0)", z[:4].tolist()))

    def report(self):
        line = "%s: %d passes, %d planted scores: worst=%.3e, worst err/bound=%.4f | %d other scores: worst rel=%.3e" % (
            self.tag, self.calls, self.rows1, self.worst1, self.ratio1, self.rows2, self.rel2)
        print(line)
        path = os.environ.get("MUSE_TEST_WORST")
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")
        assert self.calls > 0 and self.rows1 > 0 and self.rows2 > 0
        assert not self.bad, "%s: %s" % (self.tag, self.bad[:6])


def _masked_passes(muse, eng, tag, cases, occ4=False):
    """every range (the narrow ones forced through the transform) under sign 0, +1 and -1, the signed passes on rows and -rows"""
    B = muse.binding
    for ci, m in enumerate(cases):
        rep = Masked("%s N=%d n=%d f32=%d reference %d rows=%d" % (tag, m.N, m.n, m.f32, ci, len(m.rows)))
        for g in (1, -1):
            dg = muse.DeviceGroup.from_rows(eng, m.rows * g, f32=m.f32)
            db = muse.DeviceBatch(eng, dg, m.ref)
            try:
                assert db.n == m.n
                if m.f32:
                    assert np.array_equal(dg.read(0, 4), m.rows[:4] * g)
                for narrow, ranges in ((False, RS.masked_ranges(m.n)), (True, RS.FORCED_RANGES)):
                    eng.in_window_force_transform(narrow)
                    for lo, hi in ranges:
                        for s in (RS.SIGNS if g > 0 else (1, -1)):
                            got = db.scores_signed_in_lag_range(lo, hi, s) if s else db.scores_in_lag_range(lo, hi)
                            what = "[%d, %d] sign %+d %s" % (lo, hi, s, "rows" if g > 0 else "-rows")
                            if s == 0 and RS.every_lag(m.n, lo, hi):       # (every lag, no sign: the plain pass)
                                assert db.last_in_window_path() == B.MUSE_IN_WINDOW_PLAIN, what
                            else:
                                assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, (what, db.last_in_window_path())
                                name = eng.kernel_name(db)
                                assert name == RS.masked_name(m.n, m.N, m.f32, s, occ4), (what, name)
                            rep.add(what, got, m, lo, hi, s, g)
            finally:
                eng.in_window_force_transform(False)
                db.close()
                dg.close()
        rep.report()


def masked(oracle, N, f32=False):
    return _cached(("masked", N, f32), lambda: RS.masked_cases(oracle, N, f32))


@pytest.mark.parametrize("N,f32", [(N, False) for N in RS.MASKED_LENGTHS] + [(N, True) for N in RS.MASKED_F32])
def test_masked_argmax_every_index(muse, eng, oracle, N, f32):
    """a winner planted at every output index: every register and residue class of mask_window's thirty-two compares sees a 0.9
    peak just inside and just outside both bounds"""
    _masked_passes(muse, eng, "masked", masked(oracle, N, f32))


@pytest.mark.parametrize("hook,occ4", [(10, False), (7, True)])
def test_masked_argmax_every_index_forced_kernels(muse, eng, oracle, hook, occ4):
    """n = 4096: the test hooks with a masked build -- the forced default and the rescaling kernel"""
    eng.set_kernel(hook)
    try:
        _masked_passes(muse, eng, "masked hook %d" % hook, masked(oracle, 4096), occ4)
    finally:
        eng.set_kernel(0)


def test_a_hook_without_a_masked_build_refuses(muse, eng, oracle):
    B = muse.binding
    m = masked(oracle, 4096)[0]
    dg = muse.DeviceGroup.from_rows(eng, m.rows[:8])
    db = muse.DeviceBatch(eng, dg, m.ref)
    eng.set_kernel(1)
    try:
        for call in (lambda: db.score_in_lag_range(-257, 0), lambda: db.score_signed_in_lag_range(-257, 0, 1)):
            with pytest.raises(muse.MuseError) as e:
                call()
            assert e.value.status == B.MUSE_ERR_UNSUPPORTED
    finally:
        eng.set_kernel(0)
        db.close()
        dg.close()


# ------------------------------------------------------------------ d. many references
@pytest.mark.parametrize("N", RS.MANY_MASKED_LENGTHS)
def test_many_references_masked_every_index(muse, eng, oracle, N):
    """scores_many_in_lag_range over three references (code at the head, the tail and the middle) against one row set that plants
    every position: mask_window_quot at n = 4096, the small kernels' many-references build at n = 1024"""
    cases = _cached(("many-masked", N), lambda: RS.many_masked_cases(oracle, N))
    dg = muse.DeviceGroup.from_rows(eng, cases[0].rows)
    dbs = [muse.DeviceBatch(eng, dg, m.ref) for m in cases]
    reps = [Masked("many-references masked N=%d reference %d" % (N, i)) for i in range(len(cases))]
    try:
        for lo, hi in RS.MANY_MASKED_RANGES:
            got = muse.scores_many_in_lag_range(dbs, lo, hi)
            for i, m in enumerate(cases):
                assert eng.kernel_name(dbs[i]) == RS.many_masked_name(m.n, N), eng.kernel_name(dbs[i])
                reps[i].add("[%d, %d]" % (lo, hi), got[i], m, lo, hi, 0, 1)
        for rep in reps:
            rep.report()
    finally:
        for h in dbs + [dg]:
            h.close()


def test_many_references_direct_every_lag(muse, eng):
    """_winsweep.many_case(480): eight references with the code at p + offset, ranges of 127 and 101 lags from three origins, each
    batch against its own long-double table"""
    case = _cached(("many-direct",), lambda: WS.many_case(RS.MANY_N))
    tabs = _cached(("many-direct-tables",), lambda: [WS.tables(ref, case.rows, case.n, lags=RS.many_table_lags()) for ref in case.refs])
    dg = muse.DeviceGroup.from_rows(eng, case.rows)
    dbs = [muse.DeviceBatch(eng, dg, ref) for ref in case.refs]
    sws = [Sweep("many-references direct N=%d reference %d (offset %+d)" % (case.N, i, case.offsets[i])) for i in range(len(dbs))]
    try:
        for lo, hi in RS.MANY_RANGES:
            got = muse.scores_many_in_lag_range(dbs, lo, hi)
            for i in range(len(dbs)):
                assert eng.kernel_name(dbs[i]) == direct_name(case.n, case.N, lo, hi, 0), eng.kernel_name(dbs[i])
                sws[i].add("[%d, %d]" % (lo, hi), got[i], want(tabs[i], lo, hi, 0), case.outlier)
        for sw in sws:
            sw.report()
    finally:
        for h in dbs + [dg]:
            h.close()
