"""GPU tests of the many-references lag range (muse_batch_score_many_in_lag_range / _run_many_in_lag_range, run with -m gpu on an
MI355X): R references against one resident group, each series' best match inside the lags lo .. hi -- up to 48 lags the references'
table rows packed into the tiles of one fp64 matrix product (xcorr_window_many.hip with the table's origin and rows as arguments),
wider ranges one launch per reference, beyond 127 lags and on float32 storage one masked pass of the many-references transform
kernels with the two bounds set independently.

Expected values never come from the code under test: per reference and series, the definition in include/muse_hip.h applied in
numpy (tests/_lagrange.py) to the correlation slice the CPU oracle returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact except rows the ORACLE flags as
ties; tests/test_many_lag_range_cpu.py checks on the same inputs (tests/_manylagrange.py) that the oracle flags none on a
continuous-noise row, which every test here asserts again.  On the direct product the pass must also be BIT-IDENTICAL, per batch, to
that batch's own scores_in_lag_range(lo, hi)."""
import ctypes
import subprocess

import numpy as np
import pytest

import _lagrange as LR
import _lagsweep as LSW
import _manylagrange as MLR
import _window as W
from _load import pkg
from test_gpu_lag_range import SCORE_ATOL, SCORE_RTOL, check
from test_gpu_many_in_window import _assert_run

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


def inside(lag, n, lo, hi):
    lo, hi = LR.clip(n, lo, hi)
    return bool(np.all((lag >= lo) & (lag <= hi)))


def batches(muse, eng, dg, refs):
    return [muse.DeviceBatch(eng, dg, rf) for rf in refs]


def close(*hs):
    for h in hs:
        for x in (h if isinstance(h, (list, tuple)) else [h]):
            x.close()


# ------------------------------------------------------------------ 1. parity and bit-identity
@pytest.mark.parametrize("N", MLR.PARITY_NS)
def test_parity_and_bits(muse, eng, oracle, N):
    """scores_many_in_lag_range of the first R references against the oracle-derived expectation per reference, and bit for bit
    against each batch's own scores_in_lag_range, in both orders of doing the two forms: an odd row stride (N = 1433: the 8-byte
    loads), N below one chunk, two chunks with a short last one, FFT length 8192; block counts with partial 16-row blocks"""
    ref, rows, refs = MLR.case(N)
    rows, refs = rows[:max(MLR.PARITY_MS)], refs[:max(MLR.PARITY_RS)]
    ranges = MLR.ranges_of(N)
    exps, n = MLR.expectations(oracle, refs, rows, ranges)
    keep = W.plain_rows(rows.shape[0])
    for M in MLR.PARITY_MS:
        dg = muse.DeviceGroup.from_rows(eng, rows[:M])
        dbs = batches(muse, eng, dg, refs)
        assert dbs[0].n == n
        for R in MLR.PARITY_RS:
            for k, (lo, hi) in enumerate(ranges):
                first_alone = (R + k) % 2 == 1     # both orders of the two forms
                single = [db.scores_in_lag_range(lo, hi) for db in dbs[:R]] if first_alone else None
                got = muse.scores_many_in_lag_range(dbs[:R], lo, hi)
                if single is None:
                    single = [db.scores_in_lag_range(lo, hi) for db in dbs[:R]]
                for r in range(R):
                    elag, emv, tie = exps[r][0][(lo, hi)]
                    assert not (tie[:M] & keep[:M]).any()          # continuous noise: the oracle by itself yields no tie
                    check(got[r][0], got[r][1], elag[:M], emv[:M], tie[:M],
                          tag="many N=%d M=%d R=%d [%d, %d] ref=%d" % (N, M, R, lo, hi, r))
                    assert inside(got[r][0], n, lo, hi), (N, M, R, lo, hi, r)
                    assert same_bits(got[r], single[r]), (N, M, R, lo, hi, r)
                    assert dbs[r].lag_window() == -1
        close(dbs, dg)


# ------------------------------------------------------------------ 2. the packing is taken; several launches
def test_packing_is_really_taken(muse, eng):
    """the planner's table at N = 1024: every batch of a packed launch names xcorr_window_many_mfma with the launch's tiles; 16
    references at [-7, 0] fit the one launch that takes eight at +-7; 49 rows are one launch of the single-reference kernel each"""
    N, M = 1024, 100
    ref, rows, refs = MLR.case(N, M)
    refs = refs + MLR.third_refs(ref, N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    assert len(dbs) == 16
    for (Wd, R), want in MLR.PLAN_TABLE.items():
        lo, hi = -(Wd - 1), 0
        plan = muse.window_many_plan_rows(R, Wd)
        got = muse.scores_many_in_lag_range(dbs[:R], lo, hi)
        names = [eng.kernel_name(db) for db in dbs[:R]]
        for r in range(R):
            refs_l, tiles = want[int(plan["launch_of"][r])]
            if refs_l > 1:
                assert names[r].startswith("xcorr_window_many_mfma<%d, true>" % tiles), (Wd, R, r, names[r])
            else:
                assert Wd == 49 and names[r].startswith("xcorr_window_mfma<4, "), (Wd, R, r, names[r])
            assert dbs[r].last_run_path() == 0 and dbs[r].lag_window() == -1
        for r in range(R):                                           # (R = 16: the bits against the single passes are the check)
            assert same_bits(got[r], dbs[r].scores_in_lag_range(lo, hi)), (Wd, R, r)
            assert inside(got[r][0], 1024, lo, hi)
    muse.score_many_in_lag_range(dbs[:2], 0, 7)
    assert eng.kernel_name(dbs[0]).startswith("xcorr_window_many_mfma<1, true>")
    dbs[0].scores()                                                  # a plain pass behind it names the plain kernel again
    assert not eng.kernel_name(dbs[0]).startswith("xcorr_window")
    assert eng.kernel_name(dbs[1]).startswith("xcorr_window_many_mfma")
    close(dbs, dg)


@pytest.mark.parametrize("N", [1433, 4096])
def test_several_launches(muse, eng, oracle, N):
    """R = 12 references at [-15, 0] are 192 packed rows: two launches (8 + 4 references); at [-31, 0] three launches of four.
    Parity and bit-identity hold across the cuts, and a repeat gives the same bytes"""
    M = 200
    ref, rows, refs = MLR.case(N)
    rows = rows[:M]
    ranges = ((-15, 0), (-31, 0))
    exps, n = MLR.expectations(oracle, refs, rows, ranges)
    keep = W.plain_rows(M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    for (lo, hi), launches in zip(ranges, (2, 3)):
        assert muse.window_many_plan_rows(12, hi - lo + 1)["launches"] == launches
        got = muse.scores_many_in_lag_range(dbs, lo, hi)
        again = muse.scores_many_in_lag_range(dbs, lo, hi)
        for r in range(12):
            elag, emv, tie = exps[r][0][(lo, hi)]
            assert not (tie & keep).any()
            check(got[r][0], got[r][1], elag, emv, tie, tag="launches N=%d [%d, %d] ref=%d" % (N, lo, hi, r))
            assert same_bits(got[r], again[r])
            assert same_bits(got[r], dbs[r].scores_in_lag_range(lo, hi)), (N, lo, hi, r)
    close(dbs, dg)


# ------------------------------------------------------------------ 3. the cached tables do not leak between the forms
def test_tables_do_not_leak(muse, eng):
    """one list through symmetric, range and single calls in turn: every result has the bits of the same call on fresh batches"""
    N, M, R = 1024, 100, 4
    ref, rows, refs = MLR.case(N, M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs[:R])

    def fresh(fn):
        fb = batches(muse, eng, dg, refs[:R])
        try:
            return fn(fb)
        finally:
            close(fb)

    steps = (lambda bs: muse.scores_many_windowed(bs, 7),
             lambda bs: muse.scores_many_in_lag_range(bs, -7, 0),
             lambda bs: [bs[1].scores_in_window(7)],
             lambda bs: muse.scores_many_in_lag_range(bs, 0, 7),
             lambda bs: muse.scores_many_in_lag_range(bs, -7, 0))
    for k, step in enumerate(steps):
        got, want = step(dbs), fresh(step)
        assert len(got) == len(want)
        for r in range(len(got)):
            assert same_bits(got[r], want[r]), (k, r)
    close(dbs, dg)


def test_symmetric_calls_keep_their_bits(muse, eng):
    N, M, R = 1024, 100, 4
    ref, rows, refs = MLR.case(N, M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    a, b = batches(muse, eng, dg, refs[:R]), batches(muse, eng, dg, refs[:R])
    for L in (0, 7, 63, 200):
        want = muse.scores_many_in_window(a, L)
        got = muse.scores_many_in_lag_range(b, -L, L)
        for r in range(R):
            assert same_bits(got[r], want[r]), (L, r)
            assert a[r].last_in_window_path() == b[r].last_in_window_path()
            assert eng.kernel_name(a[r]) == eng.kernel_name(b[r])
    close(a, b, dg)


# ------------------------------------------------------------------ 4. the masked pass
@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", LR.MASKED_NS)
def test_masked_parity(muse, eng, oracle, N, f32):
    """ranges wider than 127 lags (float32 storage: narrow ones too), R = 4: ONE masked many-references pass where
    many_in_window_plan says so, the specials through the redo kernel with the range kept; float32 at n <= 2048 the single calls"""
    B = muse.binding
    R = MLR.MASKED_R
    ref, rows, refs = MLR.masked_case(N, f32)
    refs = refs[:R]
    n = LSW.fft_len(N)
    ranges = LR.masked_ranges(n, f32)
    exps, n2 = MLR.expectations(oracle, refs, rows, ranges)
    assert n2 == n
    keep = W.plain_rows(rows.shape[0])
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    dbs = batches(muse, eng, dg, refs)
    one_pass = 0
    for lo, hi in ranges:
        plan = muse.many_lag_range_plan(N, f32, lo, hi, R)
        got = muse.scores_many_in_lag_range(dbs, lo, hi)
        for r in range(R):
            elag, emv, tie = exps[r][0][(lo, hi)]
            assert not (tie & keep).any()
            check(got[r][0], got[r][1], elag, emv, tie, tag="masked N=%d f32=%d [%d, %d] ref=%d" % (N, f32, lo, hi, r))
            assert inside(got[r][0], n, lo, hi) and dbs[r].lag_window() == -1 and dbs[r].last_run_path() == 0
        if plan == B.MUSE_IN_WINDOW_PLAIN:                            # (n = 512: -255 .. 256 is every lag)
            assert n == 512 and LR.clip(n, lo, hi) == (-255, 256)
            continue
        assert plan == muse.many_in_window_plan(N, f32, 200, R) and plan in (B.MUSE_IN_WINDOW_MASKED, B.MUSE_IN_WINDOW_MASKED_EACH)
        for r in range(R):
            assert dbs[r].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, (N, f32, lo, hi, r)
            name = eng.kernel_name(dbs[r])
            if plan == B.MUSE_IN_WINDOW_MASKED:
                want = "xcorr_fused_n4096_fold_multi<" if n == 4096 else "xcorr_fused_small<%d, " % (n.bit_length() - 1)
                assert name.startswith(want) and name.endswith("true>"), name
                assert n == 4096 or ", true, false, true>" in name, name
            else:                                                     # float32 at n <= 2048: the single calls
                assert f32 and n <= 2048 and name.startswith("xcorr_fused_small<") and "true, true>" in name, name
                assert same_bits(got[r], dbs[r].scores_in_lag_range(lo, hi))
        if plan == B.MUSE_IN_WINDOW_MASKED:
            one_pass += 1
            if n == 4096:
                assert len(dbs[0].redo_pairs()) > 0                   # the specials went through the rescaling kernel, range kept
    assert one_pass == (0 if f32 and n <= 2048 else len(ranges) - (n == 512))
    close(dbs, dg)


# ------------------------------------------------------------------ 5. edges from planted winners
@pytest.mark.parametrize("N,rng", MLR.EDGE_CASES)
def test_edges_from_planted_winners(muse, eng, oracle, N, rng):
    """a code planted at the lags lo-1, lo, lo+1, -1, 0, 1, hi-1, hi, hi+1, three references rolled by 0, +1, -1 (a roll by s moves
    every lag by +s): inside the range the planted lag comes back, outside the result is the definition's on the oracle's cc"""
    lo, hi = rng
    ref, rows, n, planted = LR.edge_case(N, lo, hi)
    refs = [np.roll(ref, s) for s in MLR.EDGE_ROLLS]
    exps, _ = MLR.expectations(oracle, refs, rows, (rng,))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    got = muse.scores_many_in_lag_range(dbs, lo, hi)
    for r, s in enumerate(MLR.EDGE_ROLLS):
        lag, mv = got[r]
        elag, emv, tie = exps[r][0][rng]
        assert not tie.any()
        check(lag, mv, elag, emv, tie, tag="edges N=%d [%d, %d] roll %d" % (N, lo, hi, s))
        hit = 0
        for row, pl in enumerate(planted):
            if lo <= int(pl) + s <= hi:
                assert lag[row] == int(pl) + s, (N, rng, s, row, lag[row], pl)
                hit += 1
            else:
                assert lo <= int(lag[row]) <= hi, (N, rng, s, row, lag[row], pl)
        assert hit >= 5
        assert same_bits(got[r], dbs[r].scores_in_lag_range(lo, hi))
    close(dbs, dg)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_as_it_was(muse, eng):
    B = muse.binding
    L = B.load()
    rng = np.random.default_rng(8)

    def setup(N, M=6, f32=False, R=3):
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        dbs = [muse.DeviceBatch(eng, dg, rng.standard_normal(N)) for _ in range(R)]
        return dg, dbs

    def state(dbs):
        return [(db.read_scores(), db.last_in_window_path(), eng.kernel_name(db), db.lag_window()) for db in dbs]

    def refused(dbs, fn, status):
        before = state(dbs)
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message, e.value
        for (s0, p0, k0, w0), (s1, p1, k1, w1) in zip(before, state(dbs)):
            assert same_bits(s0, s1) and (p0, k0, w0) == (p1, k1, w1)

    dg, dbs = setup(1024)
    muse.score_many_in_lag_range(dbs, -7, 0)                         # (an origin other than the default to leave alone)
    muse.score_many_in_lag_range(dbs[:2], -300, 20)
    assert L.muse_batch_score_many_in_lag_range(None, 2, -7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_lag_range(None, 2, None, 0, -7, 0, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    arr = (ctypes.c_void_p * 2)(dbs[0]._h, dbs[1]._h)
    before = state(dbs)
    assert L.muse_batch_score_many_in_lag_range(arr, 0, -7, 0) == B.MUSE_ERR_INVALID                  # R = 0
    for (s0, p0, k0, w0), (s1, p1, k1, w1) in zip(before, state(dbs)):
        assert same_bits(s0, s1) and (p0, k0, w0) == (p1, k1, w1)
    refused(dbs, lambda: muse.score_many_in_lag_range([dbs[0], dbs[1], dbs[0]], -7, 0), B.MUSE_ERR_INVALID)
    for lo, hi in ((1, 7), (-7, -1), (1, 0), (0, -1)):
        refused(dbs, lambda: muse.score_many_in_lag_range(dbs, lo, hi), B.MUSE_ERR_INVALID)
        refused(dbs, lambda: muse.run_many_in_lag_range(dbs, lo, hi), B.MUSE_ERR_INVALID)
    refused(dbs, lambda: muse.run_many_in_lag_range(dbs, -7, 0, sign_filter=2), B.MUSE_ERR_INVALID)
    refused(dbs, lambda: muse.run_many_in_lag_range(dbs, -7, 0, group_id=np.zeros(6, dtype=np.int32), G=-1), B.MUSE_ERR_INVALID)
    dbs[1].set_lag_window(7)                                         # one member with a window of its own
    dbs[1].scores()
    for lo, hi in ((-7, 0), (0, 7), (-200, 7)):
        refused(dbs, lambda: muse.score_many_in_lag_range(dbs, lo, hi), B.MUSE_ERR_INVALID)
    assert dbs[1].lag_window() == 7
    dbs[1].set_lag_window(-1)
    eng.set_kernel(11)                                               # a forced kernel without a masked build: refused, not run unmasked
    try:
        refused(dbs, lambda: muse.score_many_in_lag_range(dbs, -200, 0), B.MUSE_ERR_UNSUPPORTED)
    finally:
        eng.set_kernel(0)
    got = muse.scores_many_in_lag_range(dbs, -200, 0)
    assert all(db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED for db in dbs) and all(inside(g[0], 1024, -200, 0) for g in got)
    close(dbs, dg)
    for N, f32, (lo, hi) in ((5000, False, (-200, 0)), (5000, True, (-7, 0)), (70000, False, (0, 7))):
        dg, dbs = setup(N, M=3, f32=f32, R=2)
        for db in dbs:
            db.scores()
        refused(dbs, lambda: muse.score_many_in_lag_range(dbs, lo, hi), B.MUSE_ERR_UNSUPPORTED)
        refused(dbs, lambda: muse.run_many_in_lag_range(dbs, lo, hi), B.MUSE_ERR_UNSUPPORTED)
        close(dbs, dg)


# ------------------------------------------------------------------ 7. the Run forms
@pytest.mark.parametrize("N", MLR.RUN_NS)
def test_run_many_in_lag_range_matches_the_selection_on_the_definition(muse, eng, oracle, N):
    """run_many_in_lag_range ungrouped and grouped by host equals the oracle's Results.Update / Fetch fed with the definition's
    per-row pairs of every reference; RunManyInLagRange of the Python mirror agrees; RunMany and Run behind it are what they were"""
    M, hosts, R = MLR.RUN_M, 6, MLR.RUN_R
    ref, rows, refs = MLR.run_case(N)
    exps, n = MLR.expectations(oracle, refs, rows, MLR.RUN_RANGES)
    keep = W.plain_rows(M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = batches(muse, eng, dg, refs)
    gid = (np.arange(M) % hosts).astype(np.int32)
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    for lo, hi in MLR.RUN_RANGES:
        L = max(-lo, hi)
        for r in range(R):
            assert not (exps[r][0][(lo, hi)][2] & keep).any()
        for sign, thr in ((0, 0.0), (1, 0.0), (-1, 0.0), (0, 0.35)):
            for g, Gn in ((None, 0), (gid, hosts)):
                got = muse.run_many_in_lag_range(dbs, lo, hi, g, Gn, 20, thr, sign, True)
                for r in range(R):
                    wlag, wmv, _ = exps[r][0][(lo, hi)]
                    _assert_run(got[r][0], got[r][1], got[r][2], oracle.results(wlag, wmv, g, Gn, True, L, 20, thr, sign), wmv)
                    assert dbs[r].last_run_path() == 0 and dbs[r].lag_window() == -1
        results = [muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY) for _ in range(R)]
        bs = [muse.NewBatch(muse.NewSeries(refs[r], muse.NewLabels({"graph": "ref%d" % r})), comp, results[r], 8, engine=eng)
              for r in range(R)]
        for by, g, Gn in ((None, None, 0), (["host"], gid, hosts)):
            muse.RunManyInLagRange(bs, by, lo, hi)
            for r in range(R):
                wlag, wmv, _ = exps[r][0][(lo, hi)]
                got, mean = results[r].Fetch()
                want = oracle.results(wlag, wmv, g, Gn, True, L, 12, 0.0, 0)
                assert len(got) == len(want[0]) > 0
                _assert_run([int(s.Labels.labels["i"]) for s in got], [s.Lag for s in got], [s.PercentScore for s in got], want, wmv)
        muse.RunMany(bs, None)                                        # RunMany and Run are the Runs they were
        for r in range(R):
            got, _ = results[r].Fetch()
            want = oracle.results(exps[r][1], exps[r][2], None, 0, True, L, 12, 0.0, 0)
            _assert_run([int(s.Labels.labels["i"]) for s in got], [s.Lag for s in got], [s.PercentScore for s in got], want, exps[r][2])
        bs[0].Run(None)
        got, _ = results[0].Fetch()
        oi, ol, osc, _ = oracle.results(exps[0][1], exps[0][2], None, 0, True, L, 12, 0.0, 0)
        assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
    close(dbs, dg)


def test_cpp_batch_run_many_in_lag_range(muse, oracle):
    """Batch::RunManyInLagRange of the C++ host mirror (host/muse_many_lag_range_test.cpp), in a fresh process, Fetches what the
    oracle gives for every reference"""
    exe = muse.build.build_many_lag_range_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "many lag-range ok" in r.stdout, r.stdout + r.stderr
    refs, rows = MLR.cpp_case()
    M = MLR.CPP_M
    exps, _ = MLR.expectations(oracle, refs, rows, MLR.CPP_RANGES)
    for lo, hi in MLR.CPP_RANGES:
        for k in range(MLR.CPP_R):
            wlag, wmv, tie = exps[k][0][(lo, hi)]
            assert not tie.any()
            for case, gid, G in (("nil", None, 0), ("graph", (np.arange(M) // 6).astype(np.int32), M // 6)):
                key = "%s[%d,%d]%d " % (case, lo, hi, k)
                lines = [l.split() for l in r.stdout.splitlines() if l.startswith(key)]
                want = oracle.results(wlag, wmv, gid, G, True, 300, 12, 0.0, 0)
                assert len(lines) == len(want[0]) == 12
                _assert_run([int(l[1]) for l in lines], [int(l[2]) for l in lines], [float(l[3]) for l in lines], want, wmv)


# ------------------------------------------------------------------ 8. many workgroups
def test_many_workgroups(muse, eng, oracle):
    """20 000 x 480 synthetic rows (1250 workgroups of the packed product), R = 4: 64 sampled rows per reference against the oracle on
    both paths, every row bit for bit against the single passes where the arithmetic is the same (the direct product)"""
    B = muse.binding
    M, N, R = 20000, 480, 4
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    refs = MLR.make_refs(ref, N, 1000 + N)[:R]
    dbs = batches(muse, eng, dg, refs)
    ranges = ((-7, 0), (0, 200))
    got = {}
    for lo, hi in ranges:
        got[(lo, hi)] = muse.scores_many_in_lag_range(dbs, lo, hi)
        for r in range(R):
            lag, mv = got[(lo, hi)][r]
            assert np.all((lag >= lo) & (lag <= hi)) and np.all(np.abs(mv[~np.isnan(mv)]) <= 1.0 + 1e-9)
            single = dbs[r].scores_in_lag_range(lo, hi)
            print("many workgroups [%d, %d] ref %d: %d lags and %d score bit patterns differ from the single pass"
                  % (lo, hi, r, int(np.sum(lag != single[0])), int(np.sum(mv.view(np.int64) != single[1].view(np.int64)))))
            assert same_bits(got[(lo, hi)][r], single), (lo, hi, r)
    assert eng.kernel_name(dbs[0]).startswith("xcorr_fused_small<9, ") and dbs[0].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
    starts = np.sort(np.random.default_rng(1).choice(M // 16, 4, replace=False)) * 16
    starts[-1] = M - 16                                              # (the last workgroup)
    for s0 in starts:                                                # 4 x 16 = 64 sampled rows
        rows = dg.read(int(s0), 16)
        exps, _ = MLR.expectations(oracle, refs, rows, ranges)
        for k in ranges:
            for r in range(R):
                elag, emv, tie = exps[r][0][k]
                assert int(tie.sum()) == 0
                check(got[k][r][0][s0:s0 + 16], got[k][r][1][s0:s0 + 16], elag, emv, tie, tag="rows %d.. [%d, %d] ref %d" % (s0, k[0], k[1], r))
    close(dbs, dg)
