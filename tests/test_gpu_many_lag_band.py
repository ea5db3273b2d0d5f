"""GPU tests of the many-references lag band (muse_batch_score_many_in_lag_band / _run_many_in_lag_band, run with -m gpu on an
MI355X): R references against one resident group, each series' best match inside a band of lags that need not hold lag 0, by
magnitude or under a sign -- up to 48 lags the references' table rows packed into the tiles of one fp64 matrix product
(xcorr_window_many_signed_mfma), wider bands one launch per reference, beyond 127 lags one masked pass of the many-references
transform kernels (xcorr_fused_n4096_fold_multi_band at FFT length 4096 on either storage, xcorr_fused_small_many_band at 512 ...
2048 on float64), and the single calls reference by reference on float32 storage below 4096.

Expected values never come from the code under test: per reference and series, the definition in include/muse_hip.h applied in
numpy (tests/_lagband.py) to the correlation slice the CPU oracle returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are tests/test_gpu_lag_band.py's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact on EVERY row:
tests/test_many_lag_band_cpu.py checks on the same inputs (tests/_manylagband.py) that the oracle flags no tie.  On the direct
product the pass must also be BIT-IDENTICAL, per batch, to that batch's own scores_in_lag_band(lo, hi, sign).

Where the plan says MASKED_EACH (float32 storage at FFT lengths 512 ... 2048) the call IS the single call per batch: there the result
has the bits of each batch's own scores_in_lag_band and the two invariants of the masked pass are held against the single range
calls.  The n = 4096 many-references kernel is not the single one: its results agree with a batch's own single call to the score
tolerance, not bit for bit (as for the many-references range pass), so the bit comparisons against single calls leave it out."""
import ctypes
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LSW
import _manylagband as MLB
import _manylagrange as MLR
import _signed as SG
from _load import pkg
from test_gpu_lag_band import SCORE_ATOL, SCORE_RTOL, _assert_run, _same_selection, check

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
    return muse.get_engine(0)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def batches(muse, eng, dg, refs):
    return [muse.DeviceBatch(eng, dg, rf) for rf in refs]


def close(*hs):
    for h in hs:
        for x in (h if isinstance(h, (list, tuple)) else [h]):
            x.close()


def state(eng, dbs):
    return [(db.read_scores(), db.last_in_window_path(), eng.kernel_name(db), db.lag_window()) for db in dbs]


def refused(muse, eng, dbs, fn, status):
    before = state(eng, dbs)
    with pytest.raises(muse.MuseError) as e:
        fn()
    assert e.value.status == status and e.value.message, e.value
    for (s0, p0, k0, w0), (s1, p1, k1, w1) in zip(before, state(eng, dbs)):
        assert same_bits(s0, s1) and (p0, k0, w0) == (p1, k1, w1)


def delegates(lo, hi, s):
    return s == 0 and lo <= 0 <= hi


def packed_name(muse, R, r, Wd, s, band):
    """(head, tail) of the kernel name of batch r of a packed launch of the list, or None where the planner leaves it alone in its launch"""
    plan = muse.window_many_plan_rows(R, Wd)
    l = int(plan["launch_of"][r])
    if int(np.sum(plan["launch_of"] == l)) == 1:
        return None
    return "xcorr_window_many_signed_mfma<%d, " % int(plan["tiles_of"][l]), ", %d, %s>" % (s, "true" if band else "false")


def named(name, want):
    """(the rows' alignment decides the kernel's second argument)"""
    return name.startswith(want[0]) and name.endswith(want[1]) and name[len(want[0]):-len(want[1])] in ("true", "false")


# ------------------------------------------------------------------ 1. the direct product
def _direct(muse, eng, oracle, N, M, Rs, bands):
    B = muse.binding
    ref, rows, refs = MLB.case(N)
    rows, refs = rows[:M], refs[:max(Rs)]
    exps, n = MLB.expectations(oracle, refs, rows, bands)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    assert dbs[0].n == n
    for db in dbs:
        db.scores()
    none = packed = 0
    for R in Rs:
        for k, (lo, hi) in enumerate(bands):
            c = LB.clip(n, lo, hi)
            for s in MLB.SIGNS:
                if c is None:                                        # (the far bands at n = 128)
                    refused(muse, eng, dbs[:R], lambda: muse.score_many_in_lag_band(dbs[:R], lo, hi, s), B.MUSE_ERR_INVALID)
                    continue
                assert muse.many_lag_band_plan(N, False, lo, hi, s, R) == B.MUSE_IN_WINDOW_MFMA
                first_alone = (R + k + s) % 2 == 1                   # both orders of the two forms
                single = [db.scores_in_lag_band(lo, hi, s) for db in dbs[:R]] if first_alone else None
                got = muse.scores_many_in_lag_band(dbs[:R], lo, hi, s)
                names = [eng.kernel_name(db) for db in dbs[:R]]
                paths = [db.last_in_window_path() for db in dbs[:R]]
                if single is None:
                    single = [db.scores_in_lag_band(lo, hi, s) for db in dbs[:R]]
                for r in range(R):
                    tag = "many direct N=%d M=%d R=%d [%d, %d] sign %+d ref=%d" % (N, M, R, lo, hi, s, r)
                    none += check(got[r][0], got[r][1], exps[r][(lo, hi, s)], n, (lo, hi), s, tag)
                    assert same_bits(got[r], single[r]), tag
                    assert dbs[r].lag_window() == -1 and dbs[r].last_run_path() == 0
                    if delegates(lo, hi, s):
                        continue
                    want = packed_name(muse, R, r, c[1] - c[0] + 1, s, not c[0] <= 0 <= c[1])
                    if want:
                        packed += 1
                        assert named(names[r], want) and paths[r] == 0, (tag, names[r], paths[r])
                    else:                                            # alone in its launch: named as the single call names it
                        assert paths[r] == B.MUSE_IN_WINDOW_MFMA and names[r].startswith("xcorr_window_"), (tag, names[r])
    close(dbs, dg)
    return none, packed, n


@pytest.mark.parametrize("N", MLB.DIRECT_NS)
def test_direct_product_packed_scan(muse, eng, oracle, N):
    """every band x sign for R = 1, 2, 3, 6 against the definition and bit for bit against each batch's own scores_in_lag_band, in
    both orders of the two calls: N below one chunk, an odd row length (the 8-byte loads), a short last chunk; W = 1 ... 127"""
    none, packed, n = _direct(muse, eng, oracle, N, MLB.M, MLB.DIRECT_RS, MLB.BANDS)
    assert none >= 4 and packed > 100                                # (the constant row, rows with no value of the sign)


@pytest.mark.parametrize("M", MLB.SMALL_MS)
def test_direct_product_row_counts(muse, eng, oracle, M):
    _direct(muse, eng, oracle, MLB.SMALL_M_N, M, (2, 6), MLB.BANDS)


def test_direct_product_sixteen_references_in_a_tile(muse, eng, oracle):
    """R = 16 and 17 at W = 1 (sixteen references' rows in one tile) and W = 2, and R = 12 across the launch cuts of W = 16 (8 + 4
    references) and W = 32 (three launches of four): the definition, and each batch's own single call bit for bit"""
    N = 480
    ref, rows, refs = MLB.case(N)
    refs = list(refs) + MLR.third_refs(ref, N) + [np.roll(ref, 3)]
    assert len(refs) == 17
    bands = MLB.NARROW_BANDS + MLB.CUT_BANDS
    exps, n = MLB.expectations(oracle, refs, rows, bands)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    assert muse.window_many_plan_rows(12, 16)["launches"] == 2 and muse.window_many_plan_rows(12, 32)["launches"] == 3
    assert muse.window_many_plan_rows(16, 1)["launches"] == 1 and muse.window_many_plan_rows(17, 2)["launches"] == 1
    for Rs, bs in (((16, 17), MLB.NARROW_BANDS), ((12,), MLB.CUT_BANDS)):
        for R in Rs:
            for lo, hi in bs:
                for s in MLB.SIGNS:
                    got = muse.scores_many_in_lag_band(dbs[:R], lo, hi, s)
                    names = [eng.kernel_name(db) for db in dbs[:R]]
                    again = muse.scores_many_in_lag_band(dbs[:R], lo, hi, s)
                    for r in range(R):
                        tag = "tile N=%d R=%d [%d, %d] sign %+d ref=%d" % (N, R, lo, hi, s, r)
                        check(got[r][0], got[r][1], exps[r][(lo, hi, s)], n, (lo, hi), s, tag)
                        assert same_bits(got[r], again[r]) and same_bits(got[r], dbs[r].scores_in_lag_band(lo, hi, s)), tag
                        assert named(names[r], packed_name(muse, R, r, hi - lo + 1, s, True)), (tag, names[r])
    close(dbs, dg)


# ------------------------------------------------------------------ 2. the masked pass
RANGES_WITH_ZERO = ((-200, 0), (0, 300), (-64, 300))


def _masked_many_name(n, s, band):
    head = "xcorr_fused_n4096_fold_multi_band<" if n == 4096 else "xcorr_fused_small_many_band<%d, " % (n.bit_length() - 1)
    return head, ", %d, %s>" % (s, "true" if band else "false")


def one_pass_plan(n, f32):
    return MLB.MASKED if (n == 4096 or not f32) else MLB.MASKED_EACH


@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", MLB.MASKED_NS)
def test_masked_pass(muse, eng, oracle, N, f32):
    """bands wider than 127 lags (float32 storage: narrow ones too), R = 2 and 4, every sign: ONE masked many-references pass where
    the plan says so (FFT length 4096, and 512 ... 2048 on float64: at n = 4096 the specials go through the rescaling kernel with the
    band and the sign kept), the single calls otherwise (bit for bit); the narrow bands again under
    muse_test_in_window_force_transform; and the two invariants, bit for bit: a row whose unsigned range winner has the sign gets
    that (lag, value) from the signed call, a row whose [0, hi] / [lo, 0] winner lies inside the band gets that call's bits"""
    B = muse.binding
    ref, rows, refs = MLB.masked_case(N, f32)
    refs = refs[:max(MLB.MASKED_RS)]
    n = LSW.fft_len(N)
    bands = LB.masked_bands(n) + list(LB.MASKED_FORCED)
    exps, n2 = MLB.expectations(oracle, refs, rows, bands + list(RANGES_WITH_ZERO))
    assert n2 == n
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    dbs = batches(muse, eng, dg, refs)
    un = batches(muse, eng, dg, refs)
    one_pass = each = kept_sign = kept_band = 0
    for R in MLB.MASKED_RS:
        for force in (False, True):
            eng.in_window_force_transform(force)
            try:
                for lo, hi in bands:
                    c = LB.clip(n, lo, hi)
                    for s in MLB.SIGNS:
                        if c is None:                                # ((257, 510) and (-512, -257) at n = 512)
                            refused(muse, eng, dbs[:R], lambda: muse.score_many_in_lag_band(dbs[:R], lo, hi, s), B.MUSE_ERR_INVALID)
                            continue
                        plan = muse.many_lag_band_plan(N, f32, lo, hi, s, R)
                        if force and plan != B.MUSE_IN_WINDOW_MFMA:
                            continue                                 # (ran on the masked passes in the first round)
                        if not force and plan == B.MUSE_IN_WINDOW_MFMA:
                            continue                                 # (test 1's)
                        want_plan = one_pass_plan(n, f32)
                        assert force or plan == want_plan, (N, f32, lo, hi, s, R, plan)
                        got = muse.scores_many_in_lag_band(dbs[:R], lo, hi, s)
                        names = [eng.kernel_name(db) for db in dbs[:R]]
                        for r in range(R):
                            tag = "many masked N=%d f32=%d R=%d force=%d [%d, %d] sign %+d ref=%d" % (N, f32, R, force, lo, hi, s, r)
                            assert dbs[r].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, tag
                            assert dbs[r].lag_window() == -1 and dbs[r].last_run_path() == 0
                            check(got[r][0], got[r][1], exps[r][(lo, hi, s)], n, (lo, hi), s, tag)
                            head, tail = _masked_many_name(n, s, True)
                            if want_plan == MLB.MASKED:              # the one pass
                                assert names[r].startswith(head) and names[r].endswith(tail), (tag, names[r])
                            else:                                    # the single calls: their kernels, their bits
                                assert "many" not in names[r] and "multi" not in names[r], (tag, names[r])
                                assert same_bits(got[r], un[r].scores_in_lag_band(lo, hi, s)), tag
                        if want_plan == MLB.MASKED and n == 4096:
                            assert len(dbs[0].redo_pairs()) > 0      # the specials went through the rescaling kernel, band and sign kept
                        one_pass += want_plan == MLB.MASKED
                        each += want_plan == MLB.MASKED_EACH
                        # invariant 2: the [0, hi] / [lo, 0] winner inside the band carries that call's bits
                        if s == 0 and R == MLB.MASKED_RS[0] and not force and (c[1] - c[0]) >= 127:
                            rlo, rhi = (0, hi) if lo > 0 else (lo, 0)
                            if want_plan == MLB.MASKED and muse.many_lag_range_plan(N, f32, rlo, rhi, R) == MLB.MASKED:
                                rng = muse.scores_many_in_lag_range(un[:R], rlo, rhi)
                            else:
                                rng = [u.scores_in_lag_range(rlo, rhi) for u in un[:R]]
                            for r in range(R):
                                inside = (rng[r][0] >= c[0]) & (rng[r][0] <= c[1]) & ~np.isnan(rng[r][1]) & (rng[r][1] != 0.0)
                                assert np.array_equal(got[r][0][inside], rng[r][0][inside]), (N, f32, lo, hi, r)
                                assert got[r][1][inside].tobytes() == rng[r][1][inside].tobytes(), (N, f32, lo, hi, r)
                                kept_band += int(inside.sum())
            finally:
                eng.in_window_force_transform(False)
        # invariant 1: under a sign, ranges that hold lag 0 -- a row whose unsigned winner has the sign keeps its (lag, value) bits
        for lo, hi in RANGES_WITH_ZERO:
            many_range = muse.many_lag_range_plan(N, f32, lo, hi, R)
            for s in (1, -1):
                plan = muse.many_lag_band_plan(N, f32, lo, hi, s, R)
                assert plan == one_pass_plan(n, f32)
                got = muse.scores_many_in_lag_band(dbs[:R], lo, hi, s)
                names = [eng.kernel_name(db) for db in dbs[:R]]
                if plan == MLB.MASKED and many_range == MLB.MASKED:
                    rng = muse.scores_many_in_lag_range(un[:R], lo, hi)
                else:
                    rng = [u.scores_in_lag_range(lo, hi) for u in un[:R]]
                for r in range(R):
                    tag = "many signed N=%d f32=%d R=%d [%d, %d] sign %+d ref=%d" % (N, f32, R, lo, hi, s, r)
                    check(got[r][0], got[r][1], exps[r][(lo, hi, s)], n, (lo, hi), s, tag)
                    if plan == MLB.MASKED:
                        head, tail = _masked_many_name(n, s, False)
                        assert names[r].startswith(head) and names[r].endswith(tail), (tag, names[r])
                    else:
                        assert same_bits(got[r], un[r].scores_in_lag_band(lo, hi, s)), tag
                    has = ~np.isnan(rng[r][1]) & (s * rng[r][1] > 0)
                    assert np.array_equal(got[r][0][has], rng[r][0][has]) and got[r][1][has].tobytes() == rng[r][1][has].tobytes(), tag
                    kept_sign += int(has.sum())
    if one_pass_plan(n, f32) == MLB.MASKED:
        assert one_pass >= 2 * 3 * 8 and each == 0
    else:
        assert each >= 2 * 3 * 8 and one_pass == 0
    assert kept_sign >= 20 and kept_band >= 10, (kept_sign, kept_band)
    for db in dbs:
        db.scores()
        assert db.last_in_window_path() == 0 and "band" not in eng.kernel_name(db)
    close(dbs, un, dg)


def test_masked_pass_handed_over_pairs_keep_the_band(muse, eng, oracle):
    """n = 4096, mixed units (sigmas far apart in most pairs): the one many-references pass lists those pairs and the rescaling kernel
    behind it redoes them for every reference of the list in its band build, band and sign kept"""
    B = muse.binding
    N, M, R = 4096, 63, 3
    ref, rows = SG.make_case(N, M, seed=15000)
    rows[9::2] *= 1e9                                                # every second plain row in other units
    refs = MLR.make_refs(ref, N, 1000 + N)[:R]
    bands = ((100, 300), (-300, -100))
    exps, n = MLB.expectations(oracle, refs, rows, bands)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    for lo, hi in bands:
        for s in MLB.SIGNS:
            assert muse.many_lag_band_plan(N, False, lo, hi, s, R) == MLB.MASKED
            got = muse.scores_many_in_lag_band(dbs, lo, hi, s)
            assert len(dbs[0].redo_pairs()) > M // 4                 # (listed once, by reference 0; redone per reference)
            for r in range(R):
                assert dbs[r].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
                head, tail = _masked_many_name(4096, s, True)
                assert eng.kernel_name(dbs[r]).startswith(head) and eng.kernel_name(dbs[r]).endswith(tail), eng.kernel_name(dbs[r])
                check(got[r][0], got[r][1], exps[r][(lo, hi, s)], n, (lo, hi), s, "hand-off [%d, %d] sign %+d ref=%d" % (lo, hi, s, r))
    close(dbs, dg)


# ------------------------------------------------------------------ 3. edges from planted winners
EDGE_PARAMS = [(N, band, False) for N, band in LB.EDGE_CASES] + [(N, band, True) for N, band in LB.EDGE_CASES if band[1] - band[0] + 1 <= 127]


@pytest.mark.parametrize("N,band,force", EDGE_PARAMS)
def test_edges_from_planted_winners(muse, eng, oracle, N, band, force):
    """a code planted at the lags lo-1, lo, lo+1, hi-1, hi, hi+1, -1, 0, 1, three references rolled by 0, +1, -1 (a roll by s moves
    every lag by +s): planted inside the band it comes back at sign 0, outside the row reports the definition's in-band answer; on
    the path the plan gives and, for the narrow bands, on the masked path as well"""
    B = muse.binding
    lo, hi = band
    ref, rows, n, planted = LB.edge_case(N, lo, hi)
    refs = [np.roll(ref, s) for s in MLR.EDGE_ROLLS]
    exps, _ = MLB.expectations(oracle, refs, rows, (band,))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    eng.in_window_force_transform(force)
    try:
        for s in MLB.SIGNS:
            got = muse.scores_many_in_lag_band(dbs, lo, hi, s)
            for r, roll in enumerate(MLR.EDGE_ROLLS):
                lag, mv = got[r]
                tag = "many edges N=%d [%d, %d] force=%d sign %+d roll %d" % (N, lo, hi, force, s, roll)
                # (0: a packed launch; more than 48 lags: alone in its launch, named as the single call names it)
                want_path = B.MUSE_IN_WINDOW_MASKED if force or hi - lo + 1 > 127 else B.MUSE_IN_WINDOW_MFMA if hi - lo + 1 > 48 else 0
                assert dbs[r].last_in_window_path() == want_path, tag
                check(lag, mv, exps[r][(lo, hi, s)], n, band, s, tag)
                hit = 0
                for row, pl in enumerate(planted):
                    if lo <= int(pl) + roll <= hi and s == 0:
                        assert lag[row] == int(pl) + roll, (tag, row, lag[row], pl)
                        hit += 1
                    elif not lo <= int(pl) + roll <= hi:
                        assert lag[row] == 0 or lo <= int(lag[row]) <= hi, (tag, row, lag[row], pl)
                assert s != 0 or hit >= 3, (tag, hit)
                if not (n == 4096 and want_path == B.MUSE_IN_WINDOW_MASKED):     # (the n = 4096 many-references kernel: to tolerance, above)
                    assert same_bits(got[r], dbs[r].scores_in_lag_band(lo, hi, s)), tag
    finally:
        eng.in_window_force_transform(False)
    close(dbs, dg)


# ------------------------------------------------------------------ 4. outcomes
@pytest.mark.parametrize("force", (False, True))
def test_outcomes_zero_band(muse, eng, oracle, force):
    """a band of exact zeros is (0, +0.0) for every reference and sign on the packed direct product; on the masked path the transform
    leaves rounding noise where the definition has zeros, so there the row is held to the score tolerance against +0.0 and to a lag
    of the band or 0, as tests/test_gpu_lag_band.py holds the single call"""
    B = muse.binding
    ref, rows, zr = LB.zeros_case()
    refs = [ref, 2.0 * ref, -ref]                                    # (zero wherever ref is: the zero row stays a band of zeros)
    exps, n = MLB.expectations(oracle, refs, rows, LB.ZEROS_BANDS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    eng.in_window_force_transform(force)
    try:
        for lo, hi in LB.ZEROS_BANDS:
            for s in MLB.SIGNS:
                got = muse.scores_many_in_lag_band(dbs, lo, hi, s)
                for r in range(len(refs)):
                    lag, mv = got[r]
                    tag = "many zeros force=%d [%d, %d] sign %+d ref=%d" % (force, lo, hi, s, r)
                    name = packed_name(muse, len(refs), r, hi - lo + 1, s, True)      # (more than 48 lags: alone in its launch)
                    assert dbs[r].last_in_window_path() == (B.MUSE_IN_WINDOW_MASKED if force else 0 if name else B.MUSE_IN_WINDOW_MFMA), tag
                    print("%s: row %d -> (%d, %.3e)" % (tag, zr, lag[zr], mv[zr]))
                    if not force:
                        assert name is None or named(eng.kernel_name(dbs[r]), name), tag
                        assert lag[zr] == 0 and mv[zr] == 0.0 and not np.signbit(mv[zr]), (tag, lag[zr], mv[zr])
                    else:
                        assert abs(mv[zr]) <= SCORE_ATOL and (lag[zr] == 0 or lo <= lag[zr] <= hi), (tag, lag[zr], mv[zr])
                        assert s * mv[zr] >= 0
                    others = np.arange(len(rows)) != zr
                    e = exps[r][(lo, hi, s)]
                    check(lag[others], mv[others], (e[0][others], e[1][others], e[2][others]), n, (lo, hi), s, tag)
    finally:
        eng.in_window_force_transform(False)
    close(dbs, dg)


@pytest.mark.parametrize("N", (1000, 4096))
def test_outcomes_specials_and_no_value_of_the_sign(muse, eng, oracle, N):
    """per reference and sign: the constant row is (0, 0.0), the NaN and the Inf rows (0, NaN), and a band with no value of the sign
    is exactly (0, +0.0), on the packed product and on the masked passes"""
    B = muse.binding
    ref, rows = LB.masked_case(N, False)
    refs = MLR.make_refs(ref, N, 1000 + N)[:3]
    n = LSW.fft_len(N)
    bands = ((3, 40), (-40, -3), (100, 300), (-300, -100))
    exps, _ = MLB.expectations(oracle, refs, rows, bands)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    none = {0: 0, 3: 0}
    for lo, hi in bands:
        for s in MLB.SIGNS:
            got = muse.scores_many_in_lag_band(dbs, lo, hi, s)
            for r in range(len(refs)):
                lag, mv = got[r]
                path = dbs[r].last_in_window_path()
                assert path == (0 if hi - lo + 1 <= 127 else B.MUSE_IN_WINDOW_MASKED)
                assert (lag[3], mv[3]) == (0, 0.0) and not np.signbit(mv[3])
                assert lag[4] == 0 and np.isnan(mv[4]) and lag[5] == 0 and np.isnan(mv[5])
                k = check(lag, mv, exps[r][(lo, hi, s)], n, (lo, hi), s, "many specials N=%d [%d, %d] sign %+d ref=%d" % (N, lo, hi, s, r))
                if s:
                    none[path] += k - 1                              # (beyond the constant row)
    assert none[0] > 0 and none[3] > 0, none
    close(dbs, dg)


# ------------------------------------------------------------------ 5. delegation
@pytest.mark.parametrize("N", (1024, 3000))
def test_delegation_is_bit_for_bit(muse, eng, N):
    """sign 0 with lag 0 inside IS scores_many_in_lag_range, and a symmetric one scores_many_in_window: the same bits, path and kernel"""
    ref, rows, refs = MLB.masked_case(N, False)
    R = 4
    dg = muse.DeviceGroup.from_rows(eng, rows)
    a, b = batches(muse, eng, dg, refs[:R]), batches(muse, eng, dg, refs[:R])
    for lo, hi in ((-7, 0), (-3, 12), (-200, 40), (0, 300)):
        want = muse.scores_many_in_lag_range(a, lo, hi)
        got = muse.scores_many_in_lag_band(b, lo, hi, 0)
        for r in range(R):
            assert same_bits(got[r], want[r]), (N, lo, hi, r)
            assert a[r].last_in_window_path() == b[r].last_in_window_path() and eng.kernel_name(a[r]) == eng.kernel_name(b[r])
    for L in (15, 200):
        want = muse.scores_many_in_window(a, L)
        got = muse.scores_many_in_lag_band(b, -L, L, 0)
        for r in range(R):
            assert same_bits(got[r], want[r]), (N, L, r)
            assert a[r].last_in_window_path() == b[r].last_in_window_path() and eng.kernel_name(a[r]) == eng.kernel_name(b[r])
    close(a, b, dg)


# ------------------------------------------------------------------ 6. the cached tables do not leak between the forms
def test_tables_do_not_leak(muse, eng):
    """one list through the packed range, packed band, single band and single range calls in several orders: every result has the
    bits of the same call on fresh batches (a band's tables and a range's of the same row count are different tables)"""
    N, M, R = 1025, 35, 4
    ref, rows, refs = MLB.case(N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs[:R])

    def fresh(fn):
        fb = batches(muse, eng, dg, refs[:R])
        try:
            return fn(fb)
        finally:
            close(fb)

    steps = (lambda bs: muse.scores_many_in_lag_range(bs, -7, 0),
             lambda bs: muse.scores_many_in_lag_band(bs, 1, 8, 0),
             lambda bs: [bs[1].scores_in_lag_band(-8, -1, 1)],
             lambda bs: muse.scores_many_in_lag_band(bs, -8, -1, 1),
             lambda bs: [bs[2].scores_in_lag_range(0, 7)],
             lambda bs: muse.scores_many_in_lag_band(bs, 0, 7, -1),
             lambda bs: muse.scores_many_in_lag_band(bs, 1, 8, 0),
             lambda bs: muse.scores_many_in_lag_range(bs, 0, 7),
             lambda bs: [bs[0].scores_in_lag_band(1, 8, 0)],
             lambda bs: muse.scores_many_in_lag_band(bs, 200, 207, -1),
             lambda bs: muse.scores_many_in_lag_range(bs, -7, 0))
    for k, step in enumerate(steps):
        got, want = step(dbs), fresh(step)
        assert len(got) == len(want)
        for r in range(len(got)):
            assert same_bits(got[r], want[r]), (k, r)
    close(dbs, dg)


# ------------------------------------------------------------------ 7. the Run form and the mirrors
@pytest.mark.parametrize("N", LB.RUN_NS)
def test_run_many_in_lag_band_is_the_single_runs(muse, eng, oracle, N):
    """run_many_in_lag_band, ungrouped and in label groups, equals the oracle's selection fed with the definition's per-series
    (lag, mv) of every reference and three single run_in_lag_band calls, for every sign; RunManyInLagBand / RunManySignedInLagBand of
    the Python mirror feed each Results what the batch's own method feeds"""
    M, R = LB.RUN_M, 3
    ref, rows = LB.run_case(N)
    refs = MLR.make_refs(ref, N, 1000 + N)[:R]
    exps, n = MLB.expectations(oracle, refs, rows, LB.RUN_BANDS)
    # label groups of three that keep rows 1 and 2 apart: they are the first reference and its negated copy, equal in magnitude at
    # every lag, so inside one group (tests/_lagband.py's run_groups) the last bit would decide which of the two is its winner
    G = M // LB.RUN_GROUP
    gid = (np.arange(M) % G).astype(np.int32)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs, un = batches(muse, eng, dg, refs), batches(muse, eng, dg, refs)
    labels = [{"trio": "t%02d" % (i % G), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    selected = 0
    for lo, hi in LB.RUN_BANDS:
        L = max(abs(lo), abs(hi))
        for s in MLB.SIGNS:
            for ab in (True, False):
                for g, Gn in ((None, 0), (gid, G)):
                    # against the oracle with room for every series (the rows hold the first reference and its negated copy:
                    # equal magnitudes, so at a top-N boundary the last bit decides which of the two stays), and with TopN = 20
                    # against the single calls, whose bits the pass has on the packed product and at n = 512
                    full = muse.run_many_in_lag_band(dbs, lo, hi, g, Gn, M, 0.0, s, ab)
                    got = muse.run_many_in_lag_band(dbs, lo, hi, g, Gn, 20, 0.0, s, ab)
                    for r in range(R):
                        wlag, wmv, tie = exps[r][(lo, hi, s)]
                        assert not tie.any()
                        _assert_run(full[r], oracle.results(wlag, wmv, g, Gn, ab, L, M, 0.0, s))
                        one = un[r].run_in_lag_band(lo, hi, g, Gn, 20, 0.0, s, ab)
                        if n == 4096 and hi - lo + 1 > 127:          # (the n = 4096 many-references kernel: the single runs to tolerance)
                            _assert_run(got[r], one)
                        else:
                            assert all(x.tobytes() == y.tobytes() for x, y in zip(got[r][:3], one[:3])), (N, lo, hi, s, ab, r)
                            assert got[r][3] == one[3] or (np.isnan(got[r][3]) and np.isnan(one[3]))    # (an empty selection has no mean)
                        assert len(got[r][0]) == min(20, len(full[r][0]))
                        assert dbs[r].last_run_path() == 0 and dbs[r].lag_window() == -1
                        selected += len(got[r][0])
        for signed, s, filt in ((False, 0, muse.SignFilter_ANY), (True, 0, muse.SignFilter_ANY), (True, 1, muse.SignFilter_POS),
                                (True, -1, muse.SignFilter_NEG)):
            results = [muse.NewResults(L, 12, 0.0, filt) for _ in range(R)]
            bs = [muse.NewBatch(muse.NewSeries(refs[r], muse.NewLabels({"trio": "ref%d" % r})), comp, results[r], 8, engine=eng)
                  for r in range(R)]
            for by, g, Gn in ((None, None, 0), (["trio"], gid, G)):
                (muse.RunManySignedInLagBand if signed else muse.RunManyInLagBand)(bs, by, lo, hi)
                for r in range(R):
                    got, mean = results[r].Fetch()
                    oi, ol, osc, omean = oracle.results(exps[r][(lo, hi, s)][0], exps[r][(lo, hi, s)][1], g, Gn, s == 0, L, 12, 0.0, s)
                    ids, lags, scores = [int(sc.Labels.labels["i"]) for sc in got], [sc.Lag for sc in got], [sc.PercentScore for sc in got]
                    _same_selection(ids, lags, scores, oi, ol, osc)
                    assert len(oi) == 0 or abs(mean - omean) < 1e-9
                    res1 = muse.NewResults(L, 12, 0.0, filt)         # what the batch's own method feeds
                    b1 = muse.NewBatch(muse.NewSeries(refs[r], muse.NewLabels({"trio": "ref%d" % r})), comp, res1, 8, engine=eng)
                    (b1.RunSignedInLagBand if signed else b1.RunInLagBand)(by, lo, hi)
                    own, _ = res1.Fetch()
                    _same_selection(ids, lags, scores, [int(sc.Labels.labels["i"]) for sc in own], [sc.Lag for sc in own],
                                    [sc.PercentScore for sc in own])
                    selected += len(got)
    assert selected > 300
    close(dbs, un, dg)


def test_cpp_batch_run_many_in_lag_band(muse, oracle):
    """Batch::RunManyInLagBand and RunManySignedInLagBand of the C++ host mirror (host/muse_many_lag_band_test.cpp), in a fresh
    process, Fetch what the oracle gives for every reference"""
    exe = muse.build.build_many_lag_band_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "many lag-band ok" in r.stdout, r.stdout + r.stderr
    refs, rows = MLR.cpp_case()
    M = MLR.CPP_M
    exps, _ = MLB.expectations(oracle, refs, rows, LB.CPP_BANDS)
    graphs = (np.arange(M) // 6).astype(np.int32)
    for s, ch in ((0, "0"), (1, "+"), (-1, "-")):
        for lo, hi in LB.CPP_BANDS:
            for k in range(MLR.CPP_R):
                wlag, wmv, tie = exps[k][(lo, hi, s)]
                assert not tie.any()
                for case, gid, G in (("nil", None, 0), ("graph", graphs, M // 6)):
                    key = "%s%s[%d,%d]%d " % (case, ch, lo, hi, k)
                    lines = [l.split() for l in r.stdout.splitlines() if l.startswith(key)]
                    oi, ol, osc, _ = oracle.results(wlag, wmv, gid, G, s == 0, 300, 12, 0.0, s)
                    assert len(lines) == len(oi), (key, len(lines), len(oi))
                    _same_selection([int(l[1]) for l in lines], [int(l[2]) for l in lines], [float(l[3]) for l in lines], oi, ol, osc)


# ------------------------------------------------------------------ 8. refusals against a snapshot
def test_refusals_leave_everything_as_it_was(muse, eng):
    """after each refusal every batch's scores, muse_test_last_in_window_path, kernel name and own window are what a snapshot in
    front of it recorded"""
    B = muse.binding
    L = B.load()
    rng = np.random.default_rng(8)

    def setup(N, M=6, f32=False, R=3):
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        dbs = [muse.DeviceBatch(eng, dg, rng.standard_normal(N)) for _ in range(R)]
        for db in dbs:
            db.scores()
        return dg, dbs

    dg, dbs = setup(1024)
    muse.score_many_in_lag_band(dbs, 1, 7, 1)                        # (a packed band pass's scores to leave alone)
    muse.score_many_in_lag_band(dbs[:2], 20, 300, -1)                # (and a masked one's)
    assert eng.kernel_name(dbs[2]).startswith("xcorr_window_many_signed_mfma<") and eng.kernel_name(dbs[0]).startswith("xcorr_fused_small_many_band<")
    arr = (ctypes.c_void_p * 3)(dbs[0]._h, None, dbs[2]._h)          # NULL in the list
    before = state(eng, dbs)
    assert L.muse_batch_score_many_in_lag_band(arr, 3, 1, 7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_score_many_in_lag_band(arr, 0, 1, 7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_score_many_in_lag_band(None, 3, 1, 7, 0) == B.MUSE_ERR_INVALID
    for (s0, p0, k0, w0), (s1, p1, k1, w1) in zip(before, state(eng, dbs)):
        assert same_bits(s0, s1) and (p0, k0, w0) == (p1, k1, w1)
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band([dbs[0], dbs[1], dbs[0]], 1, 7), B.MUSE_ERR_INVALID)
    arr = (ctypes.c_void_p * 3)(*[db._h for db in dbs])
    for lo, hi in ((7, 1), (0, -1), (-1, -7)):                       # lag_lo > lag_hi (the C call: the mirror has its own check)
        refused(muse, eng, dbs, lambda: B.check(L.muse_batch_score_many_in_lag_band(arr, 3, lo, hi, 0)), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.run_many_in_lag_band(dbs, lo, hi), B.MUSE_ERR_INVALID)
    for s in (2, -2, 7):                                             # a sign outside -1 .. 1
        refused(muse, eng, dbs, lambda: B.check(L.muse_batch_score_many_in_lag_band(arr, 3, 1, 7, s)), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, 1, 7, s), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.run_many_in_lag_band(dbs, 1, 7, sign_filter=s), B.MUSE_ERR_INVALID)
    for lo, hi in ((513, 600), (-900, -512), (600, 10 ** 6)):         # nothing of the band is left at FFT length 1024
        for s in MLB.SIGNS:
            refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, lo, hi, s), B.MUSE_ERR_INVALID)
    refused(muse, eng, dbs, lambda: muse.run_many_in_lag_band(dbs, 1, 7, group_id=np.zeros(6, dtype=np.int32), G=-1, sign_filter=1), B.MUSE_ERR_INVALID)
    dbs[1].set_lag_window(7)                                         # one member with a window of its own
    dbs[1].scores()
    for lo, hi, s in ((1, 7, 0), (-7, -1, 1), (0, 7, -1), (-200, 7, 1), (3, 5, 0)):
        refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, lo, hi, s), B.MUSE_ERR_INVALID)
    assert dbs[1].lag_window() == 7
    dbs[1].set_lag_window(-1)
    eng.set_kernel(11)                                               # a forced kernel without a masked build: refused, not run unmasked
    try:
        for s in MLB.SIGNS:
            refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, 1, 200, s), B.MUSE_ERR_UNSUPPORTED)
    finally:
        eng.set_kernel(0)
    got = muse.scores_many_in_lag_band(dbs, 1, 200, 1)
    assert all(db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED for db in dbs)
    assert all(np.all((g[0] >= 0) & (g[0] <= 200)) and np.all(g[1] >= 0) for g in got)
    close(dbs, dg)
    dg, dbs = setup(64, R=2)                                         # an empty band at n = 64
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, 100, 226, 0), B.MUSE_ERR_INVALID)
    close(dbs, dg)
    # not built: a 200-lag band at N = 5000, float32 storage outside FFT lengths 512 ... 4096, series longer than 65536 samples
    for N, f32, (lo, hi) in ((5000, False, (1, 200)), (5000, True, (1, 7)), (70000, False, (3, 5))):
        dg, dbs = setup(N, M=3, f32=f32, R=2)
        for s in MLB.SIGNS:
            refused(muse, eng, dbs, lambda: muse.score_many_in_lag_band(dbs, lo, hi, s), B.MUSE_ERR_UNSUPPORTED)
            refused(muse, eng, dbs, lambda: muse.run_many_in_lag_band(dbs, lo, hi, sign_filter=s), B.MUSE_ERR_UNSUPPORTED)
        close(dbs, dg)
