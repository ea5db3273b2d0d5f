"""GPU parity tests (run with -m gpu on an MI355X): every case goes through the
C ABI of libmuse_hip.so and is checked against the CPU oracle on byte-identical
inputs, or against the reference's own known-answer tables (tests/golden).

Tolerances (BASELINE.json north_star): correlation scores within 1e-6 relative
(absolute floor 1e-12 for scores that are exactly 0 in the oracle); lag indices
exact, except rows the oracle flags as rounding-decided ties (top-two |cc| gap
< 1e-12 relative) -- their count is asserted to be tiny.
"""
import math
import os

import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
SCORE_ATOL = 1e-12
TIE_GAP = 1e-12


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    # torch's bundled HIP runtime must come up before libmuse_hip.so's (the RCCL test below shares this process with the
    # engine; the other order leaves torch without a visible GPU).  bench.py does the same: torch.cuda first.
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return m


@pytest.fixture(scope="module")
def eng(muse):
    return muse.get_engine(0)


def _record_worst(tag, a, b):
    """MUSE_TEST_WORST=<file>: appends the worst relative difference of a kernel-vs-kernel comparison (how the measured values
    quoted beside the loosened tolerances below were obtained)"""
    path = os.environ.get("MUSE_TEST_WORST")
    if not path:
        return
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
    worst = float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0
    with open(path, "a") as f:
        f.write("%s %.3e\n" % (tag, worst))


def assert_scores_match(lag, mv, olag, omv, gap, max_ties=0):
    lag, mv, olag, omv = map(np.asarray, (lag, mv, olag, omv))
    nan_o = np.isnan(omv)
    assert np.array_equal(np.isnan(mv), nan_o)
    ok = ~nan_o
    err = np.abs(mv[ok] - omv[ok])
    tol = SCORE_RTOL * np.abs(omv[ok]) + SCORE_ATOL
    assert np.all(err <= tol), "score mismatch: worst rel %.3e" % float(np.max(err / np.maximum(np.abs(omv[ok]), 1e-300)))
    tie = (gap < TIE_GAP) & ok
    bad = (lag != olag) & ~tie
    assert not bad.any(), "lag mismatches at %s" % np.nonzero(bad)[0][:10]
    assert int(((lag != olag) & tie).sum()) <= max_ties
    return float(np.max(err / np.maximum(np.abs(omv[ok]), 1e-300))) if ok.any() else 0.0


# ------------------------------------------------ reference known-answer tables
def _check_sign(mv, sign):
    assert (mv > 0) if sign > 0 else (mv < 0) if sign < 0 else (mv == 0)


def test_golden_xcorr(eng, golden):                    # xcorr_test.go:86-202 (n = 5: direct kernel)
    for c in golden["xcorr"]["cases"]:
        cc, lag, mv = eng.xcorr(c["x"], c["y"], len(c["x"]), c["normalize"])
        if c["cc"] is None:
            assert cc is None
        else:
            assert np.max(np.abs(cc - np.array(c["cc"], float))) <= golden["xcorr"]["tol"]
        assert lag == c["idx"]
        _check_sign(mv, c["sign"])


def test_golden_xcorr_with_x(eng, golden):             # xcorr_test.go:204-286
    for c in golden["xcorr_with_x"]["cases"]:
        cc, lag, mv = eng.xcorr_with_x(c["x"], c["y"], n=len(c["x"]))
        if c["cc"] is None:
            assert cc is None
        else:
            assert np.max(np.abs(cc - np.array(c["cc"], float))) <= golden["xcorr_with_x"]["tol"]
        assert lag == c["idx"]
        _check_sign(mv, c["sign"])


def test_golden_tables_through_fft_kernel(eng, golden, oracle):
    """Same tables zero-padded to n = 8 (power of two -> LDS FFT kernel):
    checked against the oracle at n = 8 (the reference tables pin n = 5 only)."""
    for c in golden["xcorr_with_x"]["cases"]:
        cc, lag, mv = eng.xcorr_with_x(c["x"], c["y"], n=8)
        try:
            X, _ = oracle.ref_spectrum(c["x"], n=8)
        except ValueError:
            continue
        occ, olag, omv, _ = oracle.xcorr_with_x(X, c["y"], 8)
        if occ is None:
            assert cc is None
            continue
        assert np.max(np.abs(cc - occ)) <= 1e-12 and lag == olag and abs(mv - omv) <= 1e-12
    for c in golden["xcorr"]["cases"]:
        cc, lag, mv = eng.xcorr(c["x"], c["y"], 8, c["normalize"])
        occ, olag, omv = oracle.xcorr(c["x"], c["y"], 8, c["normalize"])
        if occ is None:
            assert cc is None
            continue
        assert np.max(np.abs(cc - occ)) <= 1e-12 and lag == olag and abs(mv - omv) <= 1e-12


def _compare_scores(scores, case):                     # compareScores, muse_test.go:11-39
    exp = case["expected"]
    assert len(scores) == len(exp)
    for s, e in zip(scores, exp):
        if "lag_in" in e:
            assert s.Lag in e["lag_in"]
        elif "tie_lags" in e:      # exact tie in exact arithmetic: rounding-decided in the reference too
            assert s.Lag in e["tie_lags"]
        else:
            assert s.Lag == e["lag"]
        assert abs(s.PercentScore - e["score"]) <= case["score_tol"]
        assert s.Labels.labels == e["labels"]


def _batch_case(muse, case):
    ref = muse.NewSeries(case["ref"], muse.NewLabels({"graph": "graph1"}))
    comp = [muse.NewSeries(s["y"], muse.NewLabels(s["labels"])) for s in case["comp"]]
    group = muse.NewGroup("targets")
    group.Add(*comp)
    r = case["results"]
    g = muse.NewBatch(ref, group, muse.NewResults(r["max_lag"], r["top_n"], r["threshold"], r["sign_filter"]), 10)
    g.Run(list(case["group_by"]))
    scores, _ = g.Results.Fetch()
    return scores


def test_batch_run_simple(muse, golden):               # muse_batch_test.go:9-44
    _compare_scores(_batch_case(muse, golden["batch_run_simple"]), golden["batch_run_simple"])


def test_batch_run_multidimensional(muse, golden):     # muse_batch_test.go:46-82
    _compare_scores(_batch_case(muse, golden["batch_run_multidim"]), golden["batch_run_multidim"])


def test_batch_run_with_larger_group(muse, golden):    # muse_batch_test.go:83-102
    c = golden["batch_run_larger_group"]
    ref = muse.NewSeries(c["ref"], muse.NewLabels({"graph": "graph1"}))
    group = muse.NewGroup("targets")
    group.Add(*[muse.NewSeries(s["y"], muse.NewLabels(s["labels"])) for s in c["comp"]])
    with pytest.raises(muse.MuseError) as e:
        muse.NewBatch(ref, group, muse.NewResults(10, 20, 0, muse.SignFilter_ANY), 1)
    assert e.value.status == muse.binding.MUSE_ERR_LENGTH


def test_new_batch_zero_std_reference(muse):           # muse_batch.go:39-41
    group = muse.NewGroup("targets")
    group.Add(muse.NewSeries([1, 2, 3, 4], muse.NewLabels({"graph": "a"})))
    with pytest.raises(muse.MuseError) as e:
        muse.NewBatch(muse.NewSeries([2, 2, 2, 2], None), group, muse.NewResults(10, 20, 0, 0), 1)
    assert e.value.status == muse.binding.MUSE_ERR_ZERO_STD
    assert "Invalid input query" in str(e.value)


def _muse_case(muse, case):
    ref = muse.NewSeries(case["ref"], muse.NewLabels({"graph": "graph1"}))
    r = case["results"]
    g = muse.New(ref, muse.NewResults(r["max_lag"], r["top_n"], r["threshold"], r["sign_filter"]))
    for s in case["comp"]:
        assert g.Run([muse.NewSeries(s["y"], muse.NewLabels(s["labels"]))]) is None
    scores, _ = g.Results.Fetch()
    return g, scores


def test_run_simple(muse, golden):                     # muse_test.go:41-73
    _compare_scores(_muse_case(muse, golden["muse_run_simple"])[1], golden["muse_run_simple"])


def test_run_simple_sign_filter(muse, golden):         # muse_test.go:75-104 (+ NEG on fresh inputs)
    _compare_scores(_muse_case(muse, golden["muse_run_sign_filter_pass1"])[1], golden["muse_run_sign_filter_pass1"])
    _compare_scores(_muse_case(muse, golden["muse_run_sign_filter_neg_fresh"])[1],
                    golden["muse_run_sign_filter_neg_fresh"])


def test_run_no_input(muse, golden):                   # muse_test.go:122-142
    g, scores = _muse_case(muse, golden["muse_run_no_input"])
    assert g.Run([]) is None and scores == []
    with pytest.raises(muse.MuseError):                # muse.go:68-70
        g.Run([muse.NewSeries([1.0, 2.0, 3.0], None)])


def test_example_shape_config1(muse, oracle):
    """BASELINE config 1 / example_test.go: N = 480 -> n = 512, 5 labelled series,
    Run(nil), Run(["graph"]), Run(["host"]) on one reused Results."""
    rng = np.random.default_rng(480)
    N = 480
    t = np.arange(N)

    def rect(a, c, w):
        return a * (np.abs(t - c) <= w / 2)

    ref_y = rect(1.5, 240, 10) + 0.1 * rng.standard_normal(N)
    L = lambda g, h: muse.NewLabels({"graph": g, "host": h})
    ref = muse.NewSeries(ref_y.copy(), L("CallTime99Pct", "host1"))
    comp = muse.NewGroup("comparison")
    ser = [ref,
           muse.NewSeries(rect(1.5, 242, 7) + 0.1 * rng.standard_normal(N), L("CallTime99Pct", "host2")),
           muse.NewSeries(rect(43, 240, 10) + 0.1 * rng.standard_normal(N), L("ErrorRate", "host1")),
           muse.NewSeries(0.1 + 0.1 * rng.standard_normal(N), L("ErrorRate", "host2")),
           muse.NewSeries(np.full(N, 0.125), L("ErrorRate", "host3"))]
    comp.Add(*ser)
    m = muse.NewBatch(ref, comp, muse.NewResults(15, 4, 0.0, muse.SignFilter_ANY), 2)
    assert m.n == 512
    rows = np.stack([s.y for s in ser])
    olag, omv, _ = oracle.batch_scores(ref_y, rows)
    for group_by, nrows in ((None, 4), (["graph"], 2), (["host"], 3)):
        m.Run(group_by)
        res, _ = m.Results.Fetch()
        assert len(res) == nrows
        keys = group_by or ["graph", "host"]
        gid, seen = [], {}
        for s in ser:
            gid.append(seen.setdefault(tuple(s.labels.labels[k] for k in keys), len(seen)))
        oi, ol, osc, _ = oracle.results(olag, omv, np.array(gid, np.int32), len(seen), True, 15, 4, 0.0, 0)
        assert [r.Labels.labels for r in res] == [ser[i].labels.labels for i in oi]
        assert [r.Lag for r in res] == ol.tolist()
        assert np.allclose([r.PercentScore for r in res], osc, rtol=1e-6, atol=1e-12)
    m.Run(None)
    res, _ = m.Results.Fetch()
    assert res[0].Labels.labels["host"] == "host1" and abs(res[0].PercentScore - 1.0) < 1e-9 and res[0].Lag == 0
    assert res[1].Labels.labels["graph"] == "ErrorRate" and res[1].PercentScore > 0.85 and res[1].Lag == 0
    assert res[-1].PercentScore == 0.0 and res[-1].Lag == 0           # constant line: sigma == 0


# ------------------------------------------------------- kernel vs oracle
def _rows(M, N, seed):
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    for i in range(0, M, 5):
        rows[i] += rng.uniform(-2, 2) * np.roll(ref, int(rng.integers(-N // 3, N // 3)))
    if M > 3:
        rows[1] = 4.0            # sigma == 0
        rows[2] = 2.5 * ref - 7  # perfect match
        rows[3] = -ref           # perfect anti-match
    return ref, rows


@pytest.mark.parametrize("N", [2, 3, 8, 12, 100, 480, 512, 1000, 2048, 3000, 4096, 5000, 8192, 10000, 16384, 40000, 65536])
@pytest.mark.parametrize("M", [1, 2, 7])
def test_scores_match_oracle_all_lengths(muse, eng, oracle, N, M):
    """generic kernel (LDS work buffer up to n = 8192, global scratch up to n = 65536: the long
    series of BASELINE config 5) and the tuned one at n = 4096, incl. N < n padding"""
    ref, rows = _rows(M, N, 1000 * N + M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == oracle.next_pow2(N)
    X, _ = oracle.ref_spectrum(ref)
    assert np.max(np.abs(db.spectrum() - (X[0::2] + 1j * X[1::2]))) < 1e-12
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows)
    assert_scores_match(lag, mv, olag, omv, gap)
    np.testing.assert_array_equal(dg.read(0, M), rows)      # inputs are never mutated


@pytest.mark.parametrize("N", [2049, 3000, 4095, 4096])
def test_every_kernel_variant_matches_oracle(muse, eng, oracle, N):
    """auto (0), generic radix-2 (1), the rescaling n = 4096 kernel (7) and the default n = 4096 kernel forced (10) on
    the same inputs, incl. N < n padding, sigma == 0, NaN / Inf rows and an odd row count."""
    ref, rows = _rows(65, N, N)
    rows[10, 5] = np.nan          # NaN row: (lag 0, mv NaN), must not disturb its pair partner
    rows[12, :] = np.inf
    rows[20, :] = 2.0 ** 600      # huge but exactly summable constant: sigma == 0 without overflow
    # pair partners whose sigmas are 1e50 / 1e13 / 1e-30 apart: two series share one complex transform,
    # so every kernel must rescale (or hand the pair to one that does) to keep the small one exact
    rows[30] *= 1e50
    rows[33] *= 1e13
    rows[36] *= 1e-30
    rows[39] *= 1e120
    rows[38] *= 1e-120
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == 4096
    olag, omv, gap = oracle.batch_scores(ref, rows)
    try:
        for variant in (0, 1, 7, 10):
            eng.set_kernel(variant)
            lag, mv = db.scores()
            assert math.isnan(mv[10]) and lag[10] == 0 and math.isnan(mv[12]) and lag[12] == 0, variant
            assert_scores_match(lag, mv, olag, omv, gap)
    finally:
        eng.set_kernel(0)


def test_config2_10000x4096_full_parity(muse, eng, oracle):
    """BASELINE config 2: 1 ref x 10 000 series, N = 4096, one batched launch;
    every row checked against the oracle on the bytes the GPU used."""
    M, N = 10000, 4096
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    rows = dg.read(0, M)
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
    worst = assert_scores_match(lag, mv, olag, omv, gap, max_ties=2)
    const = np.ptp(rows, axis=1) == 0
    copies = np.all(rows == ref[None, :], axis=1)
    assert const.sum() >= 3 and copies.sum() >= 3             # the workload exercises both paths
    assert np.all(mv[const] == 0) and np.all(lag[const] == 0)
    assert np.all(np.abs(mv[copies] - 1.0) < 1e-12) and np.all(lag[copies] == 0)
    assert (mv < 0).sum() > M // 10                           # sign mix
    print("config2 worst score rel err %.3e, ties %d" % (worst, int((gap < TIE_GAP).sum())))
    # Batch.Run semantics on top: label groups of 50 "hosts" per "graph"
    gid = (np.arange(M) // 50).astype(np.int32)
    for top_n, max_lag, thr, sign, absf in ((20, 15, 0.0, 0, True), (20, 2048, 0.3, 0, True),
                                            (7, 100, 0.0, -1, False), (300, 4096, 0.0, 0, True)):
        got = db.run(gid, M // 50, max_lag, top_n, thr, sign, absf)
        exp = oracle.results(olag, omv, gid, M // 50, absf, max_lag, top_n, thr, sign)
        assert got[1].tolist() == exp[1].tolist()
        assert np.allclose(got[2], exp[2], rtol=1e-6, atol=1e-12)
        distinct = len(set(np.round(exp[2], 9))) == len(exp[2])
        if distinct:
            assert got[0].tolist() == exp[0].tolist()
        # exact ties included (the planted copies all clamp to 1.0): muse_batch_run feeds its heap one Score per group in group
        # order, so the winners and their order are what the reference's feed (results.go:55-72) gives over the SAME scores
        own = oracle.results(lag, mv, gid, M // 50, absf, max_lag, top_n, thr, sign)
        assert got[0].tolist() == own[0].tolist() and got[1].tolist() == own[1].tolist() and got[2].tolist() == own[2].tolist()
    got = db.run(None, 0, 15, 20, 0.0, 0, True)               # Run(nil): each series its own group
    exp = oracle.results(olag, omv, None, 0, True, 15, 20, 0.0, 0)
    assert np.allclose(got[2], exp[2], rtol=1e-6, atol=1e-12) and got[1].tolist() == exp[1].tolist()
    own = oracle.results(lag, mv, None, 0, True, 15, 20, 0.0, 0)   # 10 000 groups of one: the planted copies tie at the top
    assert got[0].tolist() == own[0].tolist() and got[2].tolist() == own[2].tolist() and int(copies.sum()) >= 3


def test_group_semantics_edge_cases(muse, eng, oracle):
    """first-wins ties, NaN-first groups, empty groups, out-of-window lags,
    sign filters with abs scores."""
    N = 64
    rng = np.random.default_rng(5)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((40, N))
    rows[4] = rows[5] = 2 * ref + 1          # exact tie inside a group: first wins
    rows[8, 3] = np.nan                      # NaN first in its group: never replaced
    rows[13] = np.roll(ref, 20)              # strong peak outside MaxLag: dropped, not re-windowed
    rows[20] = 7.0
    gid = (np.arange(40) // 4).astype(np.int32)
    gid[36:] = 11                            # leaves group 9 with members 36.. gone -> group 9 empty
    G = 12
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows)
    assert_scores_match(lag, mv, olag, omv, gap)
    for top_n in (3, 12, 300):
        for sign in (0, 1, -1):
            for absf in (True, False):
                got = db.run(gid, G, 10, top_n, 0.0, sign, absf)
                exp = oracle.results(olag, omv, gid, G, absf, 10, top_n, 0.0, sign)
                assert got[0].tolist() == exp[0].tolist(), (top_n, sign, absf)
                assert got[1].tolist() == exp[1].tolist()
                assert np.allclose(got[2], exp[2], rtol=1e-6, atol=1e-12)
    got = db.run(gid, G, 10, 12, 0.0, 0, True)
    assert 4 in got[0] and 5 not in got[0] and 13 not in got[0] and 8 not in got[0]
    s, l, sc, mean = db.run(gid, G, 10, 0, 0.0, 0, True)
    assert len(s) == 0 and math.isnan(mean)


def test_device_topn_path_large_group_count(muse, eng, oracle):
    """more than 65 536 groups (EXACT_FEED_MAX_GROUPS) exercise the on-device top-N pre-selection kernel; fewer take the
    per-group feed (3 000 interleaved groups)."""
    M, N = 140000, 64
    rng = np.random.default_rng(9)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::7] += np.roll(ref, 2) * rng.uniform(0.5, 3, (len(rows[::7]), 1))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=4)
    assert_scores_match(lag, mv, olag, omv, gap)
    gid = (np.arange(M) % 3000).astype(np.int32)          # interleaved groups
    gid2 = (np.arange(M) % 70000).astype(np.int32)        # ... and more of them than the per-group feed takes
    for args in ((None, 0), (gid, 3000), (gid2, 70000)):
        for top_n in (1, 20, 256):
            got = db.run(args[0], args[1], 5, top_n, 0.1, 0, True)
            exp = oracle.results(olag, omv, args[0], args[1], True, 5, top_n, 0.1, 0)
            assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
            assert np.allclose(got[2], exp[2], rtol=1e-6, atol=1e-12)
            assert abs(got[3] - exp[3]) < 1e-9
    # sharded form: two half shards + host merge == single run
    half = M // 2
    recs = []
    for off in (0, half):
        dgs = muse.DeviceGroup.from_rows(eng, rows[off:off + half])
        dbs = muse.DeviceBatch(eng, dgs, ref)
        recs.append(dbs.run_shard(None, 0, off, 5, 20, 0.1, 0, True))
    s, l, sc, mean = muse.merge_records(np.concatenate(recs), 20)
    exp = oracle.results(olag, omv, None, 0, True, 5, 20, 0.1, 0)
    assert s.tolist() == exp[0].tolist() and l.tolist() == exp[1].tolist()


def test_invariances(muse, eng):
    """size-independent properties of z-normalized correlation: affine
    invariance of y, score 1 at the injected shift, sign flip symmetry."""
    N = 4096
    rng = np.random.default_rng(77)
    ref = rng.standard_normal(N)
    base = rng.standard_normal((32, N))
    rows = np.concatenate([base, 3.0 * base + 11.0, -base, np.stack([np.roll(ref, -k) for k in range(-8, 9)])])
    db = muse.DeviceBatch(eng, muse.DeviceGroup.from_rows(eng, rows), ref)
    lag, mv = db.scores()
    assert np.allclose(mv[:32], mv[32:64], rtol=1e-9) and np.array_equal(lag[:32], lag[32:64])
    assert np.allclose(mv[:32], -mv[64:96], rtol=1e-12) and np.array_equal(lag[:32], lag[64:96])
    assert np.array_equal(lag[96:], np.arange(-8, 9)) and np.allclose(mv[96:], 1.0, atol=1e-12)


def test_full_size_1m_x_4096_properties(muse, eng, oracle):
    """BASELINE config 3 shape (1 M x 4096 = 32.8 GB resident): sampled rows vs
    the oracle, plus properties that need no oracle at full size."""
    M, N = 1_000_000, 4096
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    assert np.all(np.abs(mv) <= 1.0 + 1e-9) and np.all(np.abs(lag) <= N // 2)
    rng = np.random.default_rng(1)
    starts = np.sort(rng.choice(M // 256, 16, replace=False)) * 256
    for s0 in starts:                                       # 16 x 256 = 4096 sampled rows
        rows = dg.read(int(s0), 256)
        olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
        assert_scores_match(lag[s0:s0 + 256], mv[s0:s0 + 256], olag, omv, gap, max_ties=1)
    zero = mv == 0
    assert 500 < zero.sum() < 1500 and np.all(lag[zero] == 0)            # ~1/1024 constant rows
    ones = np.abs(mv - 1.0) < 1e-12
    assert 500 < ones.sum() < 1500 and np.all(lag[ones] == 0)            # ~1/1024 copies of ref
    lag2, mv2 = db.scores()                                              # idempotent: inputs not mutated
    assert np.array_equal(lag, lag2) and np.array_equal(mv, mv2)
    got = db.run(None, 0, 15, 20, 0.0, 0, True)
    assert np.all(np.diff(got[2]) <= 0) and np.all(np.abs(got[2] - 1.0) < 1e-12) and np.all(got[1] == 0)
    gid = (np.arange(M) // 50).astype(np.int32)
    got = db.run(gid, M // 50, 15, 20, 0.0, 0, True)
    exp = oracle.results(lag, mv, gid, M // 50, True, 15, 20, 0.0, 0)   # host semantics on GPU scores
    assert got[1].tolist() == exp[1].tolist() and np.array_equal(got[2], exp[2])


def test_cpp_host_mirror_reference_tests(muse):
    """the reference's driver tests restated in C++ over the C ABI (host/muse_host_test.cpp)"""
    import subprocess
    exe = muse.build.build_host_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all host tests passed" in r.stdout


def test_periodic_series_many_near_ties(muse, eng, oracle):
    """periodic series have many lags whose |cc| is within rounding of the maximum: scores must match, lags outside
    the oracle-flagged ties too (every n = 4096 kernel)."""
    N = 4096
    t = np.arange(N)
    rng = np.random.default_rng(12)
    ref = np.sin(2 * np.pi * t / 64.0) + 0.01 * rng.standard_normal(N)
    rows = np.stack([np.sin(2 * np.pi * (t + s) / 64.0) + 0.01 * rng.standard_normal(N) for s in range(12)]
                    + [rng.standard_normal(N) for _ in range(5)])
    db = muse.DeviceBatch(eng, muse.DeviceGroup.from_rows(eng, rows), ref)
    olag, omv, gap = oracle.batch_scores(ref, rows)
    try:
        for variant in (0, 7, 1):
            eng.set_kernel(variant)
            lag, mv = db.scores()
            assert_scores_match(lag, mv, olag, omv, gap)
    finally:
        eng.set_kernel(0)


@pytest.mark.parametrize("N", [512, 1000, 4096, 5000, 16384, 20000, 65536])
def test_config5_mixed_lengths_label_grouped(muse, eng, oracle, N):
    """BASELINE config 5 (every length class, 512 ... 65536): one (ref, Group) pair per series length
    (the reference has no mixed-length Group: group.go:45-51, muse_batch.go:24-28), label
    groups of 10 hosts per graph, Batch.Run(["graph"]) through the host mirror, checked
    against the oracle's Batch.Run/Results semantics.  N = 1000 / 5000 are zero-padded to
    1024 / 8192, N = 20000 to 32768 (xcorr.go:176-181); the powers of two are circular (no padding)."""
    rng = np.random.default_rng(N)
    graphs, hosts = 40, 10
    t = np.arange(N)
    ref_y = 1.5 * (np.abs(t - N // 2) <= 5) + 0.1 * rng.standard_normal(N)
    ref = muse.NewSeries(ref_y, muse.NewLabels({"graph": "ref", "host": "h0"}))
    comp = muse.NewGroup("comparison")
    series, rows, gid = [], [], []
    for g in range(graphs):
        for h in range(hosts):
            amp = rng.uniform(-3, 3)
            y = amp * (np.abs(t - N // 2 - rng.integers(-20, 21)) <= rng.integers(2, 12)) + 0.1 * rng.standard_normal(N)
            if g == 7 and h == 3:
                y = 2.0 * ref_y + 1.0                     # perfect match inside a group
            if g == 9:
                y = np.full(N, 0.25)                      # a whole graph of constant lines
            series.append(muse.NewSeries(y, muse.NewLabels({"graph": "g%02d" % g, "host": "h%d" % h})))
            rows.append(y)
            gid.append(g)
    comp.Add(*series)
    res = muse.NewResults(15, 12, 0.0, muse.SignFilter_ANY)
    b = muse.NewBatch(ref, comp, res, 8)
    assert b.n == oracle.next_pow2(N)
    b.Run(["graph"])
    got, mean = res.Fetch()
    olag, omv, gap = oracle.batch_scores(ref_y, np.stack(rows))
    oi, ol, osc, omean = oracle.results(olag, omv, np.array(gid, np.int32), graphs, True, 15, 12, 0.0, 0)
    assert [s.Lag for s in got] == ol.tolist()
    assert np.allclose([s.PercentScore for s in got], osc, rtol=1e-6, atol=1e-12)
    assert [s.Labels.labels for s in got] == [series[i].labels.labels for i in oi]
    assert abs(mean - omean) < 1e-9
    assert got[0].Labels.labels == {"graph": "g07", "host": "h3"} and abs(got[0].PercentScore - 1.0) < 1e-9


@pytest.mark.parametrize("sharded", [False, True])
def test_config5_mixed_lengths_one_shared_results(muse, eng, oracle, sharded):
    """BASELINE configs[4] as ONE workload: a mixed-length Group is realised the way the reference must realise it (one length per
    Group: group.go:45-51, muse_batch.go:24-28) -- six (ref, Group) pairs, N in {512, 1000, 4096, 5000, 16384, 65536},
    2 000 series each in 200 graphs x 10 hosts, every Batch Run(["graph"]) into ONE shared Results (results.go:55-72 keeps one
    top-N heap across Runs: example_test.go:53-80 reuses one Results for three Runs), ONE Fetch at the end.  Checked against the
    oracle's Results over the union of all six Groups' oracle scores, fed in the same order (batch by batch, group by group):
    descending order, lags, scores, labels, mean |score|.  sharded: every Group cut over a list of contexts (device 0
    twice plus every other device of the box), the same Scores."""
    lengths = (512, 1000, 4096, 5000, 16384, 65536)
    graphs, hosts = 200, 10
    res = muse.NewResults(15, 20, 0.0, muse.SignFilter_ANY)
    engines = None
    if sharded:
        ndev = muse.device_count()
        engines = [muse.Engine(d) for d in ([0, 0] + list(range(1, ndev)))]
    all_lag, all_mv, all_gid, all_labels, batches = [], [], [], [], []
    for k, N in enumerate(lengths):
        rng = np.random.default_rng(1000 + N)
        t = np.arange(N)
        ref_y = 1.5 * (np.abs(t - N // 2) <= 5) + 0.1 * rng.standard_normal(N)
        M = graphs * hosts
        shift = rng.integers(-20, 21, size=(M, 1))
        width = rng.integers(2, 12, size=(M, 1))
        amp = rng.uniform(-3, 3, size=(M, 1))
        # (the noise grows with the length so that the best scores of all six lengths interleave in one top-20)
        rows = amp * (np.abs(t[None, :] - N // 2 - shift) <= width) + (0.1 + 0.02 * k) * rng.standard_normal((M, N))
        rows[1000 + 17 * k + 3] = (2.0 + k) * ref_y - 1.0   # a perfect match in every Group: six ties at 1.0 across Runs
        rows[10 * (3 + k):10 * (4 + k)] = 0.5               # a whole graph of constant lines (sigma == 0: score 0, lag 0)
        labels = [{"len": str(N), "graph": "g%03d" % (i // hosts), "host": "h%d" % (i % hosts)} for i in range(M)]
        comp = muse.NewGroup("comparison-%d" % N)
        comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
        ref = muse.NewSeries(ref_y, muse.NewLabels({"len": str(N), "graph": "ref"}))
        b = muse.NewBatch(ref, comp, res, 8, engine=eng, engines=engines)
        assert b.n == oracle.next_pow2(N)
        b.Run(["graph"])                                     # every Batch into the ONE Results
        batches.append(b)
        olag, omv, gap = oracle.batch_scores(ref_y, rows, nthreads=16)
        all_lag.append(olag)
        all_mv.append(omv)
        all_gid.append(np.arange(M, dtype=np.int32) // hosts + k * graphs)
        all_labels += labels
    got, mean = res.Fetch()                                  # ONE Fetch over all six Runs
    oi, ol, osc, omean = oracle.results(np.concatenate(all_lag), np.concatenate(all_mv), np.concatenate(all_gid),
                                        graphs * len(lengths), True, 15, 20, 0.0, 0)
    assert len(got) == 20 == len(oi)
    assert [s.Lag for s in got] == ol.tolist()
    assert np.allclose([s.PercentScore for s in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    # labels in Fetch order; among equal scores (the six planted 1.0s, equal to rounding) the order Fetch returns is the heap's own history
    # (results.go:55-87) -- in the reference that history follows Go's map iteration order (group.go:83: unspecified), here the
    # per-Batch candidates are fed in group order: compared as a set inside a run of equal scores, in order everywhere else
    want = [all_labels[i] for i in oi]
    have = [s.Labels.labels for s in got]
    k = 0
    while k < 20:
        e = k
        while e + 1 < 20 and abs(osc[e + 1] - osc[e]) <= 1e-12:   # (equal to rounding: 1.0 against 1 - 2e-16 is a tie too)
            e += 1
        key = lambda d: sorted(d.items())
        assert sorted(have[k:e + 1], key=key) == sorted(want[k:e + 1], key=key), (k, e)
        k = e + 1
    assert abs(mean - omean) < 1e-9
    assert len({s.Labels.labels["len"] for s in got}) >= 4                   # the top-20 really mixes the lengths
    assert sorted(s.Labels.labels["len"] for s in got[:6]) == sorted(str(N) for N in lengths)   # the six planted matches lead
    second, mean2 = res.Fetch()                              # Fetch drains (results.go:75-87)
    assert second == [] and math.isnan(mean2)


def test_exactly_tied_scores_follow_the_reference_feed(muse, eng, oracle):
    """Results.Update keeps a full heap's minimum unless the new Score is STRICTLY greater (results.go:63), so among exactly
    tied scores what survives at the TopN boundary and the order Fetch returns are the heap's history: Batch.Run must feed one
    Score per label group in group order (muse_batch.go:124-128), not a pre-selected subset.  Thirteen label groups hold
    bit-identical pairs of series (identical pairs share one complex transform: identical bits on the GPU too) that tie at the
    top of a TopN = 8 Results; a second Batch then Runs into the SAME Results.  One device and a Group cut over three contexts
    must both return exactly what the reference's feed gives over the same per-series scores (oracle.results on the GPU's own
    scores: the heap semantics in isolation), which in turn match the oracle's scores."""
    rng = np.random.default_rng(2024)
    N, M = 512, 400
    t = np.arange(N)
    ref_y = 1.5 * (np.abs(t - N // 2) <= 5) + 0.1 * rng.standard_normal(N)

    def make_rows(seed):
        r = np.random.default_rng(seed)
        rows = r.uniform(-2, 2, size=(M, 1)) * (np.abs(t[None, :] - N // 2 - r.integers(-20, 21, size=(M, 1))) <= 6) + 0.3 * r.standard_normal((M, N))
        rows[0] = 1.2 * ref_y + 0.05 * r.standard_normal(N)       # a strong match and its pair partner ...
        for k in (7, 20, 33, 61, 62, 90, 121, 133, 150, 170, 188, 199):
            rows[2 * k:2 * k + 2] = rows[0:2]                      # ... copied bit for bit into twelve more label groups
        return rows
    rows1, rows2 = make_rows(1), make_rows(2)
    gid = (np.arange(M) // 2).astype(np.int32)                     # label groups = the pairs
    G = M // 2

    def group_of(rows, tag):
        g = muse.NewGroup("g" + tag)
        g.Add(*[muse.NewSeries(rows[i], muse.NewLabels({"batch": tag, "graph": "g%03d" % (i // 2), "host": "h%d" % (i % 2)})) for i in range(M)])
        return g
    ref = muse.NewSeries(ref_y, muse.NewLabels({"graph": "ref"}))
    want = None
    for engines in (None, [muse.Engine(0) for _ in range(3)]):
        res = muse.NewResults(N, 8, 0.0, muse.SignFilter_ANY)
        per_series = []
        for tag, rows in (("1", rows1), ("2", rows2)):
            b = muse.NewBatch(ref, group_of(rows, tag), res, 4, engine=eng, engines=engines)
            b.Run(["graph"])                                       # both Batches into ONE Results
            dg = muse.DeviceGroup.from_rows(eng, rows)
            db = muse.DeviceBatch(eng, dg, ref_y)
            per_series.append(db.scores())
            olag, omv, gap = oracle.batch_scores(ref_y, rows)
            assert_scores_match(per_series[-1][0], per_series[-1][1], olag, omv, gap)
            db.close()
            dg.close()
        got, mean = res.Fetch()
        lag = np.concatenate([p[0] for p in per_series])
        mv = np.concatenate([p[1] for p in per_series])
        oi, ol, osc, omean = oracle.results(lag, mv, np.concatenate([gid, gid + G]), 2 * G, True, N, 8, 0.0, 0)
        have = [(s.Labels.labels["batch"], s.Labels.labels["graph"], s.Labels.labels["host"], s.Lag, s.PercentScore) for s in got]
        expect = [("1" if i < M else "2", "g%03d" % ((i % M) // 2), "h%d" % (i % 2), int(l), float(v)) for i, l, v in zip(oi, ol, osc)]
        assert have == expect                                      # order, survivors at the boundary, lags, scores: bit for bit
        assert len({h[4] for h in have}) <= 2 and len(have) == 8   # (the eight really are ties: at most the two batches' values)
        assert mean == omean
        if want is None:
            want = have
        assert have == want                                        # the sharded Group returns what one device returns


def test_group_append_staging_paths(muse, eng, oracle):
    """Group.Add-style ingestion: one muse_group_append per Series (pinned double-buffered
    staging, asynchronous upload), mixed with slab appends and growth re-allocations; the
    resident matrix must read back bit-identical and score like a bulk upload."""
    rng = np.random.default_rng(99)
    M, N = 5000, 1500                      # 12 KB rows: ~2800 rows per 32 MB staging buffer
    rows = rng.standard_normal((M, N))
    ref = rng.standard_normal(N)
    dg = muse.DeviceGroup(eng, N, capacity=16)          # forces several growth steps
    i = 0
    while i < M:
        if i % 1000 == 0 and i + 300 <= M:               # a slab of 300 rows (direct path when large enough)
            dg.append(rows[i:i + 300])
            i += 300
        else:
            dg.append(rows[i])                           # per-Series append
            i += 1
    assert dg.M == M
    np.testing.assert_array_equal(dg.read(0, M), rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    big = muse.DeviceGroup.from_rows(eng, rows)
    lag2, mv2 = muse.DeviceBatch(eng, big, ref).scores()
    assert np.array_equal(lag, lag2) and np.array_equal(mv, mv2)
    dg.append(rows[:7])                                  # append after a run: next run sees the new rows
    lag3, mv3 = db.scores()
    # two series share one complex FFT, so a row's last bits depend on its pair partner
    assert len(lag3) == M + 7 and np.array_equal(lag3[M:], lag[:7])
    np.testing.assert_allclose(mv3[M:], mv[:7], rtol=1e-12, atol=0)
    assert np.array_equal(lag3[:M], lag) and np.array_equal(mv3[:M], mv)


@pytest.mark.parametrize("N", [4096, 3000, 512, 700, 1024, 1500, 2048, 6000, 8192, 10000, 16384, 32768, 20000, 65536, 40000])
@pytest.mark.parametrize("R,M", [(2, 65), (5, 300), (1, 40)])
def test_many_references_one_pass_matches_single_batches(muse, eng, oracle, R, M, N):
    """muse_batch_score_many: R references against one resident group in one pass over the rows
    (each pair transformed once, its spectrum parked in the per-workgroup scratch slice) must give
    what R separate batches give -- and what the oracle gives -- incl. NaN/Inf/constant rows and an
    odd row count (N = 3000: the leading-zero-pad build with per-reference correction tables; n = 512 ... 2048, 8192,
    16384: the half-round kernel's one-pass build; n = 32768, 65536: the four-step kernel's, from three references on)."""
    if N > 16384:
        M = min(M, 41)                                     # (the oracle's share of the time)
    rng = np.random.default_rng(1000 + R)
    rows = rng.standard_normal((M, N))
    rows[3, 100] = np.nan
    rows[8, :] = np.inf
    rows[11, :] = -7.25
    rows[14] *= 1e30              # sigmas far apart inside a pair: listed and redone per reference
    rows[17] *= 1e-20
    refs = [rng.standard_normal(N) + (np.arange(N) == 100 * r) * 30.0 for r in range(R)]
    rows[20:20 + R] = np.stack([np.roll(refs[r], 5 * r + 1) for r in range(R)])   # known lags per reference
    dg = muse.DeviceGroup.from_rows(eng, rows)
    batches = [muse.DeviceBatch(eng, dg, ref) for ref in refs]
    got = muse.scores_many(batches)
    for r in range(R):
        lag, mv = got[r]
        olag, omv, gap = oracle.batch_scores(refs[r], rows)
        assert math.isnan(mv[3]) and lag[3] == 0 and math.isnan(mv[8]) and lag[8] == 0
        assert mv[11] == 0.0 and lag[11] == 0
        assert_scores_match(lag, mv, olag, omv, gap)
        slag, smv = batches[r].scores()                 # the single-reference kernel on the same batch
        # (n = 8192, 32768, 65536: the single-reference kernel is a REAL transform of one series, the many-references pass a complex
        # transform of a pair -- two float64 evaluations of the same numbers; lags may differ where the oracle flags a tie)
        other = batches[r].n in (8192, 32768, 65536)
        assert np.array_equal(lag, slag) or (other and np.all((lag == slag) | (gap < TIE_GAP)))
        # measured worst relative difference (MUSE_TEST_WORST, round 6, one box): 0 at n = 512 ... 2048 (the same kernel), 1.4e-15 at
        # 4096, 2.7e-15 at 8192, 3.2e-15 at 16384, 1.7e-15 at 32768 / 65536 -- round 5's 1e-9 for the "other" lengths was never needed
        _record_worst("many_vs_single n=%d" % batches[r].n, mv, smv)
        np.testing.assert_allclose(mv, smv, rtol=1e-12, atol=0, equal_nan=True)
    # Run semantics for every reference in one call
    gid = (np.arange(M) // 7).astype(np.int32)
    G = int(gid.max()) + 1
    many = muse.run_many(batches, gid, G, max_lag=2048, top_n=6, threshold=0.0, sign_filter=0, abs_scores=True)
    for r in range(R):
        s1, l1, v1, m1 = batches[r].run(gid, G, 2048, 6, 0.0, 0, True)
        s2, l2, v2, m2 = many[r]
        assert np.array_equal(s1, s2) and np.array_equal(l1, l2)
        np.testing.assert_allclose(v1, v2, rtol=1e-12)
        assert abs(m1 - m2) <= 1e-12 * abs(m1)


def test_many_references_large(muse, eng):
    """200 000 x 4096 synthetic rows, 4 references: every row of every reference equals the
    single-reference result (lags exact, scores to rounding)."""
    M, N, R = 200_000, 4096, 4
    dg, ref0 = muse.DeviceGroup.synthetic(eng, M, N, seed=77)
    refs = [ref0] + [dg.read(1000 * r + 1, 1)[0] for r in range(1, R)]
    batches = [muse.DeviceBatch(eng, dg, ref) for ref in refs]
    got = muse.scores_many(batches)
    for r in range(R):
        slag, smv = batches[r].scores()
        assert np.array_equal(got[r][0], slag), r
        np.testing.assert_allclose(got[r][1], smv, rtol=1e-11, atol=0, equal_nan=True)


@pytest.mark.parametrize("N", [512, 1000, 2048, 5000, 8192, 16384, 20001, 32768, 40000, 65536])
def test_per_length_kernels_at_scale_match_the_stockham_kernels(muse, eng, oracle, N):
    """~ 0.5 GB of synthetic rows per length (several resident sets of workgroups, odd row counts, planted copies and constant
    rows): the per-length default kernels (xcorr_small.hip / xcorr_long.hip: persistent loops, rows requested one iteration
    ahead, pair lists) against round 1's independent Stockham kernels (test hook 11) on EVERY row -- lags exact, scores to
    rounding -- and against the oracle on a sample of rows."""
    M = max(1001, (1 << 29) // (8 * N)) | 1
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=4242 + N)
    db = muse.DeviceBatch(eng, dg, ref)
    try:
        lag, mv = db.scores()
        eng.set_kernel(11)
        slag, smv = db.scores()
    finally:
        eng.set_kernel(0)
    same = lag == slag
    # (near-ties between two lags may resolve differently in two implementations: a handful at most, and then the scores agree)
    assert int((~same).sum()) <= 3
    np.testing.assert_allclose(mv, smv, rtol=1e-10, atol=1e-13, equal_nan=True)
    pick = np.unique(np.concatenate(([0, 1, M - 2, M - 1], np.random.default_rng(N).integers(0, M, size=24))))
    rows = np.stack([dg.read(int(i), 1)[0] for i in pick])
    olag, omv, gap = oracle.batch_scores(ref, rows)
    assert_scores_match(lag[pick], mv[pick], olag, omv, gap, max_ties=1)
    db.close()
    dg.close()


@pytest.mark.parametrize("N", [257, 480, 512, 700, 1000, 1024, 1025, 1500, 2048,
                               4097, 5000, 6001, 8191, 8192, 10000, 16384, 16385, 20000, 24001, 32767, 32768, 32769, 40000, 50001, 65535, 65536])
def test_stockham_kernels_match_oracle_and_generic(muse, eng, oracle, N):
    """n = 512 ... 2048 (LDS) and 8192 ... 65536 (global scratch): the radix-16 Stockham kernels
    (auto / variant 11) against the oracle and the radix-2 generic kernel (variant 1) on the same
    rows, incl. N < n padding, sigma == 0, NaN / Inf rows, an odd row count and more pairs than one
    workgroup iteration holds."""
    M = 83 if N <= 4096 else 23
    ref, rows = _rows(M, N, 31 * N)
    rows[10, 5 % N] = np.nan
    rows[12, :] = np.inf
    rows[20, :] = 2.0 ** 600
    rows[14] *= 1e40              # sigmas far apart inside a pair (shared complex transform)
    rows[17] *= 1e-25
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    olag, omv, gap = oracle.batch_scores(ref, rows)
    try:
        got = {}
        small = db.n <= 2048 or db.n in (8192, 16384)   # lengths the half-round kernel (xcorr_small.hip) is built for
        variants = ((0, 11, 12, 1) if small else (0, 11, 1)) + ((13,) if db.n >= 16384 else ()) + ((14,) if db.n >= 8192 else ()) + ((15,) if db.n == 32768 else ())
        # (13: xcorr_long.hip, 14: xcorr_real.hip -- one REAL series per workgroup: n = 8192 on the 4096-point transform, n = 32768 / 65536
        # on the 16384-point one)
        for variant in variants:
            eng.set_kernel(variant)
            lag, mv = db.scores()
            assert math.isnan(mv[10]) and lag[10] == 0 and math.isnan(mv[12]) and lag[12] == 0, variant
            assert_scores_match(lag, mv, olag, omv, gap)
            got[variant] = (lag, mv)
        auto = 15 if db.n == 32768 else 14 if db.n >= 8192 else 12 if small else 11      # what automatic selection takes for this length
        assert np.array_equal(got[0][0], got[auto][0]) and np.array_equal(got[0][1], got[auto][1], equal_nan=True)
    finally:
        eng.set_kernel(0)


def test_mirror_run_many_equals_runs(muse):
    """RunMany over the reference-style API (Series / Group / Batch / Results): three references
    against one Group with Run(["graph"]) semantics == three separate Batch.Run calls."""
    rng = np.random.default_rng(5)
    N, M, R = 4096, 41, 3
    comp = muse.NewGroup("targets")
    for i in range(M):
        y = rng.standard_normal(N)
        y[1000 + 13 * i:1040 + 13 * i] += 4.0
        comp.Add(muse.NewSeries(y, muse.NewLabels({"graph": "g%d" % (i // 4), "host": "h%d" % i})))
    refs = []
    for r in range(R):
        y = rng.standard_normal(N)
        y[1500 + 100 * r:1540 + 100 * r] += 4.0
        refs.append(muse.NewSeries(y, muse.NewLabels({"graph": "ref%d" % r})))
    many = [muse.NewBatch(ref, comp, muse.NewResults(4096, 5, 0.0, muse.SignFilter_ANY), 4) for ref in refs]
    single = [muse.NewBatch(ref, comp, muse.NewResults(4096, 5, 0.0, muse.SignFilter_ANY), 4) for ref in refs]
    muse.RunMany(many, ["graph"])
    for r in range(R):
        single[r].Run(["graph"])
        a, am = many[r].Results.Fetch()
        b, bm = single[r].Results.Fetch()
        assert len(a) == len(b) == 5
        for x, y in zip(a, b):
            assert x.Lag == y.Lag and x.Labels.ID(x.Labels.Keys()) == y.Labels.ID(y.Labels.Keys())
            assert abs(x.PercentScore - y.PercentScore) <= 1e-12
        assert abs(am - bm) <= 1e-12


def test_fuzz_random_shapes_against_oracle(muse, eng, oracle):
    """Seeded sweep over random (N, M) and data regimes -- large offsets, tiny and huge scales, sparse
    spikes, constant / NaN / Inf rows -- through automatic kernel selection (every kernel family:
    generic n < 512, Stockham LDS, tuned 4096, four-step) against the oracle."""
    rng = np.random.default_rng(20261003)
    lengths = [2, 3, 5, 17, 64, 255, 256, 300, 511, 513, 777, 1023, 1100, 2000, 2047, 2049, 3333, 4095, 4096,
               4097, 6000, 8191, 8193, 12000, 16383, 16384, 16385, 30000, 32768, 50000, 65535, 65536]
    worst = 0.0
    for trial, N in enumerate(lengths):
        M = int(rng.integers(1, 12)) if N > 8192 else int(rng.integers(1, 40))
        regime = trial % 5
        ref = rng.standard_normal(N)
        rows = rng.standard_normal((M, N))
        if regime == 1:
            rows += 1e6 * rng.standard_normal((M, 1))                    # large level, unit noise
        elif regime == 2:
            rows *= 10.0 ** rng.uniform(-150, 150, size=(M, 1))          # extreme scales
        elif regime == 3:
            rows[:] = 0.0                                                # sparse spikes
            for i in range(M):
                rows[i, rng.integers(0, N, size=max(1, min(N, 3)))] = rng.standard_normal(max(1, min(N, 3)))
        elif regime == 4 and N > 4:
            rows += np.roll(ref, int(rng.integers(-N // 2, N // 2)))[None, :] * rng.uniform(-3, 3, size=(M, 1))
        if M > 2:
            rows[int(rng.integers(0, M))] = 3.25                          # sigma == 0
        if M > 4:
            rows[int(rng.integers(0, M)), int(rng.integers(0, N))] = np.nan
            rows[int(rng.integers(0, M)), int(rng.integers(0, N))] = np.inf
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        olag, omv, gap = oracle.batch_scores(ref, rows)
        worst = max(worst, assert_scores_match(lag, mv, olag, omv, gap, max_ties=2))
        db.close()
        dg.close()
    print("fuzz worst relative score error %.3e" % worst)


def test_fuzz_run_semantics_against_oracle(muse, eng, oracle):
    """Seeded sweep over Batch.Run / Muse.Run post-processing: random group maps (incl. empty groups and
    G both below and above the device top-N threshold), MaxLag, TopN, Threshold, sign filter and abs
    flag; scores are continuous random values, so no exact ties straddle the top-N boundary."""
    rng = np.random.default_rng(77)
    for trial in range(24):
        N = int(rng.choice([96, 700, 4096]))
        M = int(rng.integers(1, 6000 if N < 1000 else 1500))
        ref = rng.standard_normal(N)
        rows = rng.standard_normal((M, N))
        k = max(1, M // 7)
        for i in rng.integers(0, M, size=k):                       # planted matches at random lags / signs
            rows[i] += rng.uniform(-4, 4) * np.roll(ref, int(rng.integers(-N // 2, N // 2)))
        if M > 10:
            rows[int(rng.integers(0, M))] = 1.0                    # sigma == 0
            rows[int(rng.integers(0, M)), 0] = np.nan
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        olag, omv, gap = oracle.batch_scores(ref, rows)
        assert_scores_match(lag, mv, olag, omv, gap, max_ties=2)
        for _ in range(4):
            if rng.random() < 0.25:
                gid, G = None, 0
            else:
                G = int(rng.integers(1, max(2, 2 * M)))
                gid = rng.integers(0, G, size=M).astype(np.int32)
            max_lag = int(rng.choice([0, 3, 15, N // 4, N]))
            top_n = int(rng.choice([1, 5, 20, 257, 1000]))
            thr = float(rng.choice([0.0, 0.05, 0.3]))
            sign = int(rng.choice([0, 1, -1]))
            absf = bool(rng.random() < 0.6)
            got = db.run(gid, G, max_lag, top_n, thr, sign, absf)
            # the oracle post-processes the GPU's own (lag, mv): this test is about the selection logic
            exp = oracle.results(lag, mv, gid, G, absf, max_lag, top_n, thr, sign)
            key = (trial, N, M, G, max_lag, top_n, thr, sign, absf)
            assert got[0].tolist() == exp[0].tolist(), key
            assert got[1].tolist() == exp[1].tolist(), key
            assert np.array_equal(got[2], exp[2], equal_nan=True), key
            assert (math.isnan(got[3]) and math.isnan(exp[3])) or abs(got[3] - exp[3]) <= 1e-15 * max(1.0, abs(exp[3])), key
        db.close()
        dg.close()


@pytest.mark.parametrize("N", [1000, 4096, 5000, 16384])
def test_samples_whose_squares_overflow(muse, eng, oracle, N):
    """|x| ~ 1e250: sum (x - mean)^2 overflows.  In the reference gonum's compensation term
    (sum (x - mean))^2 / n overflows as well, the variance is Inf - Inf = NaN and every cc is NaN
    -> (0, NaN); the tuned kernels' shifted sums overflow the same way.  (Between ~1e154 and ~1e170 the
    reference's outcome depends on the rounding residue of its own summation order -- NaN or (0, 0.0) --
    and is not reproducible by any other implementation; not tested.)  The pair partner stays exact."""
    rng = np.random.default_rng(N)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((9, N))
    rows[2] *= 1e250
    rows[5] *= -1e250
    dg = muse.DeviceGroup.from_rows(eng, rows)
    lag, mv = muse.DeviceBatch(eng, dg, ref).scores()
    olag, omv, gap = oracle.batch_scores(ref, rows)
    assert math.isnan(omv[2]) and math.isnan(omv[5])
    assert_scores_match(lag, mv, olag, omv, gap)


def test_mixed_unit_group_every_pair_handed_off(muse, eng, oracle):
    """a Group that alternates O(1) and O(1e30) series (mixed-unit metrics): EVERY pair of the default
    N = 4096 kernel is listed for the rescaling kernel; results still match the oracle row by row"""
    rng = np.random.default_rng(9)
    M, N = 3001, 4096
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::5] += 2.0 * np.roll(ref, 7)[None, :]
    rows[1::2] *= 1e30
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
    assert_scores_match(lag, mv, olag, omv, gap, max_ties=1)
    # the second pass over the same rows goes to the rescaling kernel directly (automatic selection learnt the
    # hand-off count of the first): same results
    lag2, mv2 = db.scores()
    # Run(); Run() is bit-identical (the tie rules of muse_batch.go:87 are "first wins": a last-bit difference between two passes
    # could reorder a Fetch): a dense list makes the FIRST pass redo every pair with the rescaling kernel too -- the un-paired last
    # row, which is never listed, included
    assert np.array_equal(lag, lag2) and np.array_equal(mv, mv2)
    lag3, mv3 = db.scores()
    assert np.array_equal(lag, lag3) and np.array_equal(mv, mv3)
    db.close()
    dg.close()
    # a SPARSE list (one pair in sixteen: below the hand-off threshold) is followed in every pass: identical bits again
    rows = rng.standard_normal((M, N))
    rows[1::32] *= 1e30
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
    assert_scores_match(lag, mv, olag, omv, gap, max_ties=1)
    for _ in range(2):
        lag2, mv2 = db.scores()
        assert np.array_equal(lag, lag2) and np.array_equal(mv, mv2)
    db.close()
    dg.close()


@pytest.mark.parametrize("N", [8, 12, 480, 1000, 4096, 5000, 20000])
def test_run_rows_one_call_equals_run_groups(muse, eng, oracle, N):
    """muse_batch_run_rows (Muse.Run, muse.go:46-92, as one ABI call through a pooled slot) against muse_batch_run_groups over
    an uploaded group of the same rows, and against the reference loop over the oracle's scores: signed and abs scores, one to
    1 001 series, a NaN first member (never replaced), a NaN later member, a constant series, exact ties (the first wins), a
    row stride wider than N, groups of different sizes and lengths alternating on the same slots, an empty group."""
    rng = np.random.default_rng(400 + N)
    ref_y = rng.standard_normal(N)
    probe = muse.DeviceGroup(eng, N, 0)
    tmpl = muse.DeviceBatch(eng, probe, ref_y)
    X, n = oracle.ref_spectrum(ref_y)
    for case, M in enumerate((1, 2, 5, 50, 1001 if N <= 4096 else 65, 3)):
        wide = np.zeros((M, N + 5))
        rows = wide[:, :N] if case % 2 else np.zeros((M, N))         # (odd cases: row_stride = N + 5)
        rows[:] = rng.standard_normal((M, N))
        rows[::3] += np.roll(ref_y, 1) * rng.uniform(-3, 3, (len(rows[::3]), 1))
        if M >= 5:
            rows[3] = rows[1]                                          # exact tie: the earlier series keeps the group
            rows[4] = 0.5                                              # sigma == 0: score 0
        if case == 3:
            rows[0, N // 2] = np.nan                                   # the FIRST member scores NaN: the group's score is NaN
        if case == 4:
            rows[2, 1] = np.nan                                        # a later NaN member is skipped
        dg = muse.DeviceGroup.from_rows(eng, np.ascontiguousarray(rows))
        db = muse.DeviceBatch.like(tmpl, dg)
        olag, omv, gap = oracle.batch_scores(ref_y, np.ascontiguousarray(rows)) if not np.isnan(rows).any() else (None, None, None)
        for abs_scores in (False, True):
            eng.rows_always_copy(True)                                 # both ways in: through the copy ...
            copied = tmpl.run_rows(rows, abs_scores=abs_scores)
            eng.rows_always_copy(False)                                # ... and (up to 256 KB) read by the kernel from pinned memory
            win, st = tmpl.run_rows(rows, abs_scores=abs_scores)
            assert copied[1] == st and copied[0].tolist() == win.tolist()
            rec, state = db.run_groups(np.zeros(M, dtype=np.int32), 1, 0, abs_scores=abs_scores)
            assert st == int(state[0]) and win.tolist() == rec[0].tolist(), (N, M, abs_scores)
            assert st == (2 if case == 3 else 1)
            if olag is not None:                                       # the reference loop (muse.go:64-88) over the oracle's scores
                sc = np.minimum(np.abs(omv), 1.0) if abs_scores else np.clip(omv, -1.0, 1.0)
                best = 0
                for i in range(1, M):
                    if abs(sc[i]) > abs(sc[best]) + (1e-9 if abs(abs(sc[i]) - abs(sc[best])) < 1e-9 else 0.0):
                        best = i
                assert abs(win["score"] - sc[best]) <= SCORE_RTOL * abs(sc[best]) + SCORE_ATOL
                if gap[int(win["series"])] >= TIE_GAP and int(win["series"]) == best:
                    assert int(win["lag"]) == int(olag[best])
                if M >= 5:
                    assert int(win["series"]) != 3                     # (series 3 repeats series 1 bit for bit and never wins)
        db.close()
        dg.close()
    win, st = tmpl.run_rows(np.zeros((0, N)))
    assert st == 0 and int(win["series"]) == -1
    with pytest.raises(muse.MuseError) as ei:
        tmpl.run_rows(np.zeros((2, max(N - 1, 1))))
    assert ei.value.status == muse.binding.MUSE_ERR_LENGTH
    tmpl.close()
    probe.close()


def test_run_rows_large_group_takes_the_general_path(muse, eng):
    """more than 2^24 samples do not fit a slot: the same entry point uploads a group and runs it (same record)"""
    N, M = 4096, 4100
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=99, copies=False)
    rows = dg.read(0, M)
    db = muse.DeviceBatch(eng, dg, ref)
    rec, state = db.run_groups(np.zeros(M, dtype=np.int32), 1, 0, abs_scores=False)
    win, st = db.run_rows(rows, abs_scores=False)
    assert st == 1 == int(state[0]) and win.tolist() == rec[0].tolist()
    db.close()
    dg.close()


def test_muse_run_concurrent_callers(muse):
    """muse_test.go:203-214 drives one *Muse from many goroutines (Results is mutex-protected,
    results.go:12,60,71): the same from Python threads -- every call crosses the C ABI on the shared
    context with the GIL released -- must give what sequential calls give."""
    import threading
    rng = np.random.default_rng(3)
    N = 1024
    ref_y = rng.standard_normal(N)
    ref_y[400:440] += 5.0
    ref = muse.NewSeries(ref_y, muse.NewLabels({"graph": "ref"}))
    groups = []
    for g in range(24):
        ss = []
        for k in range(5):
            y = rng.standard_normal(N)
            y[(400 + 9 * g + k) % N:(440 + 9 * g + k) % N or None] += 3.0 + k
            ss.append(muse.NewSeries(y, muse.NewLabels({"graph": "g%d" % g, "host": "h%d" % k})))
        groups.append(ss)
    seq = muse.New(ref, muse.NewResults(N, 10, 0.0, muse.SignFilter_ANY))
    for ss in groups:
        seq.Run(ss)
    par = muse.New(ref, muse.NewResults(N, 10, 0.0, muse.SignFilter_ANY))
    errors = []

    def work(chunk):
        try:
            for ss in chunk:
                par.Run(ss)
        except Exception as e:          # pragma: no cover
            errors.append(e)
    threads = [threading.Thread(target=work, args=(groups[i::6],)) for i in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    a, am = seq.Results.Fetch()
    b, bm = par.Results.Fetch()
    key = lambda s: (round(abs(s.PercentScore), 12), s.Lag, s.Labels.ID(s.Labels.Keys()))
    assert sorted(map(key, a)) == sorted(map(key, b))
    assert abs(am - bm) <= 1e-12


def test_fuzz_padded_and_many_references(muse, eng, oracle):
    """Seeded sweep over N in (2048, 4096] (the default kernel's leading-zero-pad build and its correction
    table), data regimes incl. an outlying first sample (the shift K), and R references in one pass."""
    rng = np.random.default_rng(4242)
    for trial in range(14):
        N = int(rng.choice([2049, 2500, 3000, 3333, 4000, 4095, 4096]))
        M = int(rng.integers(2, 90))
        R = int(rng.integers(1, 5))
        rows = rng.standard_normal((M, N))
        regime = trial % 4
        if regime == 1:
            rows += 1e5 * rng.standard_normal((M, 1))
        elif regime == 2:
            rows[:, 0] += 1e4 * rng.standard_normal(M)            # the first sample (the kernel's shift) is an outlier
        elif regime == 3:
            rows *= 10.0 ** rng.uniform(-8, 8, size=(M, 1))
        if M > 6:
            rows[int(rng.integers(0, M))] = -2.0
            rows[int(rng.integers(0, M)), int(rng.integers(0, N))] = np.nan
        refs = [rng.standard_normal(N) * (1.0 + 10.0 * r) + 3.0 * r for r in range(R)]
        for r in range(R):
            rows[r % M] += 0.5 * np.roll(refs[r], 3 + r) * np.std(rows[r % M][np.isfinite(rows[r % M])])
        dg = muse.DeviceGroup.from_rows(eng, rows)
        batches = [muse.DeviceBatch(eng, dg, ref) for ref in refs]
        got = muse.scores_many(batches)
        for r in range(R):
            olag, omv, gap = oracle.batch_scores(refs[r], rows)
            assert_scores_match(got[r][0], got[r][1], olag, omv, gap, max_ties=1)
        for b in batches:
            b.close()
        dg.close()


def test_grouped_run_sharded_on_group_boundaries(muse, eng, oracle):
    """config 4/5 shape on one GPU: a grouped Batch.Run over three shards cut by dist.shard_bounds_grouped
    (no label group straddles a shard), per-shard top-N records merged on the host == the unsharded run."""
    rng = np.random.default_rng(8)
    N = 1024
    sizes = rng.integers(1, 30, size=400)
    gid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    M, G = len(gid), len(sizes)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::11] += np.roll(ref, 4) * rng.uniform(0.5, 2.0, (len(rows[::11]), 1))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    whole = muse.DeviceBatch(eng, dg, ref).run(gid, G, 8, 25, 0.05, 0, True)
    recs = []
    for rank in range(3):
        lo, hi = muse.dist.shard_bounds_grouped(gid, 3, rank)
        if hi == lo:
            continue
        dgs = muse.DeviceGroup.from_rows(eng, rows[lo:hi])
        recs.append(muse.DeviceBatch(eng, dgs, ref).run_shard(gid[lo:hi], G, lo, 8, 25, 0.05, 0, True))
    s, l, sc, mean = muse.merge_records(np.concatenate(recs), 25)
    assert s.tolist() == whole[0].tolist() and l.tolist() == whole[1].tolist()
    np.testing.assert_allclose(sc, whole[2], rtol=1e-12)
    assert abs(mean - whole[3]) <= 1e-12


# ------------------------------------------------ filter-and-refine Run (fp32 screening pass + fp64 for the rows that matter)
def _screen_cases(rng, N):
    ref = np.zeros(N)
    ref[N // 5:N // 3] = 1.0
    ref += 0.1 * rng.standard_normal(N)
    M = 17000 if N <= 8192 else 1500        # (long series: fewer rows, the tests lower the path's threshold)
    rows = rng.standard_normal((M, N))
    t = np.arange(N)
    for i in range(0, M, 3):                                        # planted matches: all lags, both signs, all strengths
        rows[i] += rng.uniform(-3, 3) * np.roll(ref - ref.mean(), int(rng.integers(-N // 2, N // 2))) * 3.0
    for i in range(100, 160):                                       # a crowd of nearly equal scores around a cut
        rows[i] = np.roll(ref, 5) + 0.3 * rows[99] + 1e-7 * (i - 100) * rng.standard_normal(N)
    for i in range(200, 230):                                       # periodic: many lags tie within any window
        rows[i] = np.sin(2 * np.pi * (t + i) / 64.0) + 0.01 * rng.standard_normal(N)   # (period 64 divides every n)
    rows[300] = ref                                                 # score 1 at lag 0
    # (exact ties in |score| are avoided: their order in the reference's heap depends on rows evicted earlier)
    rows[301] = -np.roll(ref, -12) + 0.01 * rows[301]               # score ~ -1 inside MaxLag 15
    rows[302] = np.roll(ref, 16) + 0.02 * rows[302]                 # score ~ 1 just outside MaxLag 15
    rows[303] = 4.0                                                 # sigma == 0
    rows[304, 7] = np.nan
    rows[305] = np.inf
    rows[306] = rows[306] * 1e60 + np.roll(ref, 3) * 3e60           # sigma outside the fp32 range
    rows[307] = 1e-70 * (rows[307] + 3 * np.roll(ref, -3))
    rows[308] = np.roll(ref, 2) + 0.05 * rows[308]
    rows[308, 0] += 500.0                                           # x[0] a far outlier (the fp32 shift point)
    rows[309] = 1e6 + 1e-3 * (np.roll(ref, 1) + 0.05 * rows[309])  # large offset, small variation
    return ref, rows


@pytest.mark.parametrize("N", [65536, 40000, 16384, 8192, 5000, 4096, 3000, 2048, 1500, 1024, 600, 512])
def test_screened_run_equals_fp64_run(muse, eng, oracle, N):
    """The filter-and-refine Run (muse_ctx_set_screening) returns the records of the all-fp64 Run: adversarial rows
    (near ties at the cut, periodic series, NaN / Inf / sigma == 0, sigmas outside the fp32 range, a far-outlier first
    sample) under every filter combination, for N == n and for zero-padded series, at every FFT length the path is built
    for (4096: radix-16 kernel; 2048 / 1024 / 512: fp32 Stockham kernels); the expected records are the oracle's Results
    over the fp64 scores."""
    rng = np.random.default_rng(2024)
    ref, rows = _screen_cases(rng, N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    try:
        eng.set_screening(True, min_rows=1000)
        for max_lag in (15, 0, 2048, 4096, 100):
            for top_n, thr, sign, absf in ((20, 0.0, 0, True), (1, 0.0, 0, True), (200, 0.0, 0, True), (20, 0.3, 0, True),
                                          (20, 0.0, 1, False), (20, 0.0, -1, False), (50, 0.05, -1, True),
                                          (20, 0.999, 0, True), (256, 0.0, 1, True)):
                got = db.run(None, 0, max_lag, top_n, thr, sign, absf)
                key = (max_lag, top_n, thr, sign, absf)
                # the path under test ran for EVERY combination (a costly one only switches itself off, not the batch)
                assert db.last_run_path() == 1 and db.last_run_info()[0] is True, (N, key)
                exp = oracle.results(lag, mv, None, 0, absf, max_lag, top_n, thr, sign)
                assert got[0].tolist() == exp[0].tolist(), key
                assert got[1].tolist() == exp[1].tolist(), key
                # (2048 < N < 4096 and n >= 32768: the all-scores kernel transforms x - x[0] and corrects for the mean
                # afterwards, the re-evaluating kernel centres and rescales before the transform: the two fp64 results
                # differ by ~1e-11 relative on the rows built to stress exactly that; n = 8192, 32768, 65536: the all-scores
                # kernel is a real transform of one series (xcorr_real.hip), the re-evaluating one a complex transform of a pair)
                # measured worst relative difference (MUSE_TEST_WORST, round 6, one box): 0 up to N = 2048, 2.6e-12 at N = 3000,
                # 3.5e-13 at 4096, 4.8e-13 at 5000, 1.4e-12 at 8192, 9.5e-13 at 16384, 3.8e-12 at 40000, 3.7e-12 at 65536
                loose = 2048 < N < 4096 or N > 4096
                _record_worst("screened_vs_all_scores N=%d" % N, got[2], exp[2])
                np.testing.assert_allclose(got[2], exp[2], rtol=5e-11 if loose else 1e-12, atol=0, err_msg=str(key))
        # the all-scores API after a screened Run still returns fp64 results for every row
        lag2, mv2 = db.read_scores()
        assert np.array_equal(lag2, lag)
        np.testing.assert_allclose(mv2, mv, rtol=1e-12, atol=0, equal_nan=True)
    finally:
        eng.set_screening(False)  # the default: opt-in
        db.close()


@pytest.mark.parametrize("N", [65536, 20000, 8192, 6000, 4096, 2500, 2048, 1100, 512])
def test_screening_estimates_stay_inside_the_bound(muse, eng, oracle, N):
    """|fp32 estimate - fp64 score| <= E for every series the pass did not hand to the fp64 kernel, with E the bound
    the selection assumes; the flags cover the exact lag (inside / outside MaxLag) and the exact sign."""
    rng = np.random.default_rng(7)
    ref, rows = _screen_cases(rng, N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    worst = 0.0
    for max_lag in (15, 700):
        est, flags, E = db.screen_estimates(max_lag)
        assert 0 < E < 2e-2      # (grows with sqrt(n): 1.2e-2 * max|X| at n = 65536)
        refined = (flags >> 31) & 1 == 1
        nan = np.isnan(mv)
        assert np.all((flags[nan] & 32) != 0) and np.all((flags[~nan] & 32) == 0)
        chk = ~refined & ~nan & ((flags & 16) == 0)
        err = np.abs(np.abs(est[chk]) - np.abs(mv[chk]))
        assert err.max() <= E, (err.max(), E)
        worst = max(worst, float(err.max() / E))
        inside = np.abs(lag[chk]) <= max_lag
        f = flags[chk]
        assert np.all((f[inside] & 1) != 0) and np.all((f[~inside] & 2) != 0)
        big = np.abs(mv[chk]) > 4 * E
        assert np.all((f[big & (mv[chk] > 0)] & 4) != 0) and np.all((f[big & (mv[chk] < 0)] & 8) != 0)
        assert np.all((flags[[306, 307, 308]] & 16) != 0)            # sigma out of range, outlier first sample
    print("screening: worst |estimate - exact| / E = %.3g" % worst)
    db.close()


def test_screened_run_synthetic_matches_fp64_run(muse, eng):
    """BASELINE's synthetic rect+noise rows (device generated), 131072 of them: screened Run == fp64 Run.  The
    generator plants exact copies of the reference (score exactly 1 after the clamp), so many rows tie at the top and
    which of them a Run returns depends on the last bit of each kernel's score: the comparison is on the scores, and on
    every returned row being a correct member (filters passed, exact score equal to the reported one)."""
    dg, ref = muse.DeviceGroup.synthetic(eng, 131072, 4096, seed=99)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    try:
        for args in ((None, 0, 15, 20, 0.0, 0, True), (None, 0, 4096, 100, 0.2, 0, True), (None, 0, 15, 20, 0.0, -1, False),
                     (None, 0, 40, 256, 0.0, 1, False)):
            eng.set_screening(False)
            exp = db.run(*args)
            eng.set_screening(True)
            got = db.run(*args)
            assert len(got[0]) == len(exp[0]), args
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
            rows = got[0]
            assert len(set(rows.tolist())) == len(rows)
            assert np.all(np.abs(lag[rows]) <= args[2]) and np.array_equal(lag[rows], got[1])
            exact = np.clip(np.abs(mv[rows]), None, 1.0) if args[6] else np.clip(mv[rows], -1.0, 1.0)
            np.testing.assert_allclose(got[2], exact, rtol=1e-12, atol=0)
            assert abs(got[3] - exp[3]) <= 1e-12
    finally:
        eng.set_screening(False)  # the default: opt-in
        db.close()


def test_screened_run_fuzz_filters_and_smooth_series(muse, eng, oracle):
    """Random Run parameters on two kinds of rows: white noise with planted matches (sharp correlation peaks) and
    random walks (very smooth correlation: many lags inside any window of the maximum, so few rows `certainly` pass
    the MaxLag filter and the path has to re-evaluate many rows or give the batch back to the fp64 pass)."""
    rng = np.random.default_rng(31337)
    N, M = 4096, 16500
    eng.set_screening(True, min_rows=16384)
    for kind in ("noise", "walk"):
        if kind == "noise":
            ref = rng.standard_normal(N)
            rows = rng.standard_normal((M, N))
            for i in rng.integers(0, M, size=M // 4):
                rows[i] += rng.uniform(-2, 2) * np.roll(ref, int(rng.integers(-N // 2, N // 2)))
        else:
            ref = np.cumsum(rng.standard_normal(N))
            rows = np.cumsum(rng.standard_normal((M, N)), axis=1)
            for i in rng.integers(0, M, size=M // 4):
                rows[i] += rng.uniform(-3, 3) * np.roll(ref, int(rng.integers(-40, 40)))
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        screened_runs = 0
        for trial in range(14):
            max_lag = int(rng.choice([0, 2, 15, 64, 1000, 4096]))
            top_n = int(rng.choice([1, 3, 20, 100, 256]))
            thr = float(rng.choice([0.0, 0.02, 0.1, 0.5]))
            sign = int(rng.choice([0, 1, -1]))
            absf = bool(rng.random() < 0.5)
            got = db.run(None, 0, max_lag, top_n, thr, sign, absf)
            screened_runs += int(db.last_run_info()[0])
            exp = oracle.results(lag, mv, None, 0, absf, max_lag, top_n, thr, sign)
            key = (kind, trial, max_lag, top_n, thr, sign, absf)
            assert got[0].tolist() == exp[0].tolist(), key
            assert got[1].tolist() == exp[1].tolist(), key
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0, err_msg=str(key))
        assert screened_runs >= 1, kind          # the path was exercised (it may switch itself off afterwards)
        db.close()
    eng.set_screening(False)


@pytest.mark.parametrize("N", [4096, 1000, 20000])
def test_screened_run_with_label_groups(muse, eng, oracle, N):
    """Grouped Runs (Batch.Run(groupByLabels)) on the filter-and-refine path: per-group bounds decide which members
    are re-evaluated.  Group maps from a handful of large groups to thousands of small ones, empty groups, groups
    whose first member is NaN, and every filter; expected records: the oracle's Results over the fp64 scores."""
    rng = np.random.default_rng(4242)
    M = 16600 if N <= 4096 else 2400
    eng.set_screening(True, min_rows=1000)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    for i in rng.integers(0, M, size=M // 3):
        rows[i] += rng.uniform(-3, 3) * np.roll(ref, int(rng.integers(-N // 2, N // 2)))
    rows[5] = 2.0                    # sigma == 0
    rows[17, 100] = np.nan
    rows[400] = np.inf
    rows[900] *= 1e70                # fp32 not trusted
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    screened_runs = 0
    for trial in range(24):
        G = int(rng.choice([3, 40, 700, 5000, 20000]))
        gid = rng.integers(0, G, size=M).astype(np.int32)
        if trial % 3 == 0:
            gid[17] = gid[16]        # a NaN member that is not necessarily first
            gid[:50] = np.arange(50) % min(G, 50)
        if trial % 4 == 1:
            gid = np.sort(gid)       # contiguous groups (the layout a Go Group produces)
        max_lag = int(rng.choice([0, 15, 200, 4096]))
        top_n = int(rng.choice([1, 5, 20, 100, 256]))
        thr = float(rng.choice([0.0, 0.05, 0.3]))
        sign = int(rng.choice([0, 1, -1]))
        absf = bool(rng.random() < 0.5)
        got = db.run(gid, G, max_lag, top_n, thr, sign, absf)
        screened_runs += int(db.last_run_info()[0])
        exp = oracle.results(lag, mv, gid, G, absf, max_lag, top_n, thr, sign)
        key = (trial, G, max_lag, top_n, thr, sign, absf)
        assert got[0].tolist() == exp[0].tolist(), key
        assert got[1].tolist() == exp[1].tolist(), key
        np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0, err_msg=str(key))
    assert screened_runs >= 1
    db.close()
    eng.set_screening(False)


def test_screened_run_degenerate_inputs(muse, eng, oracle):
    """Inputs on which the screening pass can certify almost nothing: every row constant (sigma == 0: score 0 at lag
    0), every row NaN, an odd row count, a Threshold above 1, a negative MaxLag, one label group for all rows, every
    row its own copy of the reference (all scores tie at 1).  The records must still be those of the fp64 Run."""
    rng = np.random.default_rng(99)
    N, M = 4096, 16385
    eng.set_screening(True, min_rows=16384)
    ref = rng.standard_normal(N)
    cases = {}
    cases["constant rows"] = np.tile(rng.uniform(-5, 5, size=(M, 1)), (1, N))
    nanrows = rng.standard_normal((M, N))
    nanrows[:, 7] = np.nan
    cases["NaN rows"] = nanrows
    noise = rng.standard_normal((M, N))
    noise[::2] += 2.0 * ref
    cases["noise"] = noise
    cases["copies of the reference"] = np.tile(ref, (M, 1)) * rng.uniform(0.5, 2.0, size=(M, 1))
    for name, rows in cases.items():
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        one = np.zeros(M, dtype=np.int32)
        for gid, G, max_lag, top_n, thr, sign, absf in ((None, 0, 15, 20, 0.0, 0, True), (None, 0, 15, 20, 2.0, 0, True),
                                                        (None, 0, -1, 20, 0.0, 0, True), (one, 1, 15, 5, 0.0, 0, True),
                                                        (None, 0, 4096, 256, 0.0, -1, False), (one, 1, 4096, 1, 0.5, 1, False)):
            got = db.run(gid, G, max_lag, top_n, thr, sign, absf)
            exp = oracle.results(lag, mv, gid, G, absf, max_lag, top_n, thr, sign)
            key = (name, G, max_lag, top_n, thr, sign, absf)
            assert len(got[0]) == len(exp[0]), key
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0, err_msg=str(key))
            if name != "copies of the reference":       # (exact ties: which of the tied rows is returned is not defined)
                assert got[0].tolist() == exp[0].tolist(), key
                assert got[1].tolist() == exp[1].tolist(), key
            else:
                assert np.array_equal(lag[got[0]], got[1]), key
        db.close()
    eng.set_screening(False)


def test_screening_bound_guard_falls_back_to_fp64(muse, oracle):
    """The run-time guard: every re-evaluated row has an fp32 estimate and an fp64 score; if they differ by more than the
    bound the selection assumed, the Run is redone in fp64 and the batch leaves the filter-and-refine path.  Forced here
    by shrinking the assumed bound a million-fold through the test hook muse_test_set_screen_bound_scale."""
    rng = np.random.default_rng(5)
    N, M = 4096, 16500
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    for i in rng.integers(0, M, size=M // 4):
        rows[i] += rng.uniform(-2, 2) * np.roll(ref, int(rng.integers(-100, 100)))
    e2 = muse.Engine(0)
    try:
        e2.set_screen_bound_scale(1e-6)
        e2.set_screening(True, min_rows=16384)
        dg = muse.DeviceGroup.from_rows(e2, rows)
        db = muse.DeviceBatch(e2, dg, ref)
        lag, mv = db.scores()
        for args in ((None, 0, 100, 20, 0.0, 0, True), (None, 0, 4096, 5, 0.1, -1, False)):
            got = db.run(*args)
            assert db.last_run_info()[0] is False          # redone in fp64 (first Run), or not screened any more
            assert db.last_run_path() == 3                  # ... because the guard tripped
            exp = oracle.results(lag, mv, None, 0, args[6], args[2], args[3], args[4], args[5])
            assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
        db.close()
    finally:
        e2.close()


def test_screened_run_many_references(muse, eng, oracle):
    """muse_batch_run_many on the filter-and-refine path: one screening pass for all references (rows read and forward
    transformed once, the fp32 spectrum parked per workgroup), then keys / cut / re-evaluation per reference.  Records per
    reference = the oracle's Results over that reference's fp64 scores; with and without label groups; references of
    very different spectra (white noise, a rectangle, a slow sine) share the pass's window."""
    rng = np.random.default_rng(808)
    N, M = 4096, 16500
    t = np.arange(N)
    refs = [rng.standard_normal(N), np.where((t > 700) & (t < 1500), 1.0, 0.0) + 0.05 * rng.standard_normal(N),
            np.sin(2 * np.pi * t / 900.0) + 0.1 * rng.standard_normal(N), rng.standard_normal(N),
            np.cumsum(rng.standard_normal(N))]
    rows = rng.standard_normal((M, N))
    for i in rng.integers(0, M, size=M // 3):
        rows[i] += rng.uniform(-3, 3) * np.roll(refs[int(rng.integers(0, len(refs)))], int(rng.integers(-300, 300)))
    rows[11] = 7.0
    rows[12, 9] = np.nan
    rows[13] *= 1e80
    dg = muse.DeviceGroup.from_rows(eng, rows)
    bs = [muse.DeviceBatch(eng, dg, r) for r in refs]
    exact = [b.scores() for b in bs]
    eng.set_screening(True, min_rows=16384)
    try:
        for trial in range(8):
            R = int(rng.choice([2, 3, 5]))
            pick = [int(i) for i in rng.choice(len(refs), size=R, replace=False)]
            if trial % 2:
                G = int(rng.choice([50, 3000]))
                gid = rng.integers(0, G, size=M).astype(np.int32)
            else:
                gid, G = None, 0
            max_lag = int(rng.choice([15, 500, 4096]))
            top_n = int(rng.choice([1, 20, 100]))
            thr = float(rng.choice([0.0, 0.1]))
            sign = int(rng.choice([0, 1, -1]))
            absf = bool(rng.random() < 0.5)
            got = muse.run_many([bs[i] for i in pick], gid, G, max_lag, top_n, thr, sign, absf)
            for j, i in enumerate(pick):
                lag, mv = exact[i]
                exp = oracle.results(lag, mv, gid, G, absf, max_lag, top_n, thr, sign)
                key = (trial, i, G, max_lag, top_n, thr, sign, absf)
                assert got[j][0].tolist() == exp[0].tolist(), key
                assert got[j][1].tolist() == exp[1].tolist(), key
                np.testing.assert_allclose(got[j][2], exp[2], rtol=1e-12, atol=0, err_msg=str(key))
            if trial == 0:
                assert bs[pick[0]].last_run_info()[0] is True      # the first call, at least, took the screened path
    finally:
        eng.set_screening(False)
        for b in bs:
            b.close()


def test_run_sharded_over_rccl_world_size_1(muse, eng, oracle):
    """dist.run_sharded with backend "nccl" (= RCCL) in this process as the only rank: the device-side all_gather of
    the shard's records + merge must reproduce the unsharded Run (ungrouped and grouped), incl. a non-zero series
    offset.  (World sizes > 1: gloo tests on CPU; the 8-GPU run is the driver's.)"""
    import socket
    import torch
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        dg, ref = muse.DeviceGroup.synthetic(eng, 40000, 4096, seed=321, copies=False)   # (copies tie at 1.0: order undefined)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        gid = (np.arange(40000) // 50).astype(np.int32)
        for g, G, off in ((None, 0, 0), (None, 0, 123456), (gid, 800, 0)):
            got = muse.dist.run_sharded(db, off, g, G, 15, 20, 0.0, 0, True, device=torch.device("cuda", 0))
            exp = oracle.results(lag, mv, g, G, True, 15, 20, 0.0, 0)
            assert (got[0] - off).tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
            assert got[3] == exp[3]
        # label groups on any rank (second branch): the all_gather + exact-feed path and the all_to_all slices of a
        # Run over more than 65 536 label groups (forced), both over RCCL with device tensors; interleaved graphs, an offset
        gid2 = (np.arange(40000) % 800).astype(np.int32)
        exp = oracle.results(lag, mv, gid2, 800, True, 15, 20, 0.0, 0)
        for limit in (None, 0):
            got = muse.dist.run_grouped_sharded(db, 5000, gid2, 800, 15, 20, 0.0, 0, True, device=torch.device("cuda", 0),
                                                exact_feed_max_groups=limit, with_groups=True)
            assert (got[0] - 5000).tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
            assert got[3] == exp[3] and got[4].tolist() == gid2[exp[0]].tolist()
        db.close()
    finally:
        dist.destroy_process_group()


def test_sharded_batch_run_on_one_rank_equals_batch_run(muse, eng, oracle):
    """dist.ShardedBatch (what bench.py's config5 leg and a one-process-per-GPU host run) against the mirror's Batch.Run over the
    same series: two Batches of different lengths into ONE shared Results each way, interleaved graphs, bit-identical planted
    series in different graphs (exact ties at the top), a NaN-first graph -- the same Scores in the same order, and the
    oracle's Results over the union."""
    shared_a, shared_b = muse.NewResults(30, 9, 0.0, muse.SignFilter_ANY), muse.NewResults(30, 9, 0.0, muse.SignFilter_ANY)
    all_lag, all_mv, all_gid, base, labels = [], [], [], 0, []
    for k, (M, N, graphs) in enumerate(((900, 1000, 45), (600, 512, 30))):
        rng = np.random.default_rng(300 + k)
        t = np.arange(N)
        ref_y = 1.5 * (np.abs(t - N // 2) <= 5) + 0.1 * rng.standard_normal(N)
        rows = rng.uniform(-2, 2, size=(M, 1)) * (np.abs(t[None, :] - N // 2 - rng.integers(-20, 21, size=(M, 1))) <= 6) + 0.3 * rng.standard_normal((M, N))
        strong = 1.2 * ref_y + 0.05 * rng.standard_normal(N)
        for i in (2, 3, 100, 101, 250, 251, 444, 445, 598, 599):
            rows[i] = strong                                   # bit-identical series (pairs share one transform: identical bits)
        rows[7, 5] = np.nan                                    # first member of graph 7
        gid = (np.arange(M) % graphs).astype(np.int32)
        labs = [{"b": str(k), "graph": "g%02d" % (i % graphs), "host": "h%d" % (i // graphs)} for i in range(M)]
        comp = muse.NewGroup("c%d" % k)
        comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labs[i])) for i in range(M)])
        muse.NewBatch(muse.NewSeries(ref_y, muse.NewLabels({"graph": "ref"})), comp, shared_a, 4, engine=eng).Run(["graph"])
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref_y)
        muse.dist.ShardedBatch(db, 0, shared_b, lambda i, g, labs=labs: muse.NewLabels(labs[i])).Run(gid, graphs)
        lag, mv = db.scores()
        olag, omv, gap = oracle.batch_scores(ref_y, rows)
        assert_scores_match(lag, mv, olag, omv, gap)
        all_lag.append(lag)
        all_mv.append(mv)
        all_gid.append(gid + base)
        base += graphs
        labels += labs
        db.close()
        dg.close()
    ga, ma = shared_a.Fetch()
    gb, mb = shared_b.Fetch()
    key = lambda sc: [(s.Labels.labels, s.Lag, s.PercentScore) for s in sc]
    assert key(ga) == key(gb) and ma == mb and len(ga) == 9
    oi, ol, osc, omean = oracle.results(np.concatenate(all_lag), np.concatenate(all_mv), np.concatenate(all_gid), base, True, 30, 9, 0.0, 0)
    assert key(gb) == [(labels[i], int(l), float(v)) for i, l, v in zip(oi, ol, osc)] and mb == omean
    assert len({s.PercentScore for s in gb[:5]}) <= 2              # (the planted copies tie)


def test_costly_filters_switch_off_only_themselves(muse, eng, oracle):
    """a screened Run that re-evaluates more than a quarter of its pairs (random walks under a small MaxLag:
    almost nothing certainly passes) goes back to the fp64 pass for THOSE filters only; benign filters on the same
    batch stay on the filter-and-refine path, and every Run returns the fp64 records."""
    rng = np.random.default_rng(77)
    N, M = 4096, 16500
    ref = np.cumsum(rng.standard_normal(N))
    rows = np.cumsum(rng.standard_normal((M, N)), axis=1)
    eng.set_screening(True, min_rows=16384)
    try:
        db = muse.DeviceBatch(eng, muse.DeviceGroup.from_rows(eng, rows), ref)
        lag, mv = db.scores()
        costly = (None, 0, 2, 20, 0.0, 0, True)
        benign = (None, 0, 4096, 20, 0.0, 0, True)
        paths = []
        for args in (costly, benign, costly, benign):
            got = db.run(*args)
            paths.append(db.last_run_path())
            exp = oracle.results(lag, mv, None, 0, args[6], args[2], args[3], args[4], args[5])
            assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist(), args
        assert paths[0] == 1 and db.last_run_info is not None
        assert paths[1] == 1 and paths[3] == 1, paths          # benign filters: screened before and after
        if paths[2] != 1:                                        # the costly Run did hand itself back ...
            assert paths[2] == 2, paths                          # ... for being costly, nothing else
        db.close()
    finally:
        eng.set_screening(False)


def test_scores_many_after_a_screened_run_is_one_pass(muse, eng, oracle):
    """the one-pass many-references kernel leaves exact fp64 scores in every batch, so reading them back
    after an earlier screened Run must not re-score batch by batch (launch count of the timed pass = 1)."""
    rng = np.random.default_rng(5150)
    N, M, R = 4096, 16500, 3
    rows = rng.standard_normal((M, N))
    refs = [rng.standard_normal(N) for _ in range(R)]
    dg = muse.DeviceGroup.from_rows(eng, rows)
    bs = [muse.DeviceBatch(eng, dg, r) for r in refs]
    eng.set_screening(True, min_rows=16384)
    try:
        for b in bs:
            b.run(None, 0, 15, 20, 0.0, 0, True)
            assert b.last_run_info()[0] is True
        eng.kernel_time()
        eng.kernel_timing(True)
        got = muse.scores_many(bs)
        eng.synchronize()
        eng.kernel_timing(False)
        ms, launches = eng.kernel_time()
        assert launches == 1, launches
        for r in range(R):
            olag, omv, gap = oracle.batch_scores(refs[r], rows)
            assert_scores_match(got[r][0], got[r][1], olag, omv, gap)
    finally:
        eng.set_screening(False)
        for b in bs:
            b.close()


@pytest.mark.parametrize("N", [512, 1024, 2048, 3000, 4096, 8192, 16384, 65536])
def test_screening_error_on_adversarial_inputs(muse, eng, oracle, N):
    """docs/screen_error_bound.md section 5: inputs built to maximise the fp32 pass's error -- +-1 sequences (no
    cancellation anywhere), chirps (flat spectra), single spikes, |mean d| just inside the 8 sigma limit (first sample
    a far outlier), variance mantissas just below 2 with ODD exponents in both series of a pair (scl * sigma -> 2: the
    largest ||z||_2 the scaling allows), periodic rows with many near-tie lags -- against a reference with a large
    max|X| (a sine: one dominant bin).  Worst |estimate - exact| over every row the pass vouches for: <= E / 8."""
    rng = np.random.default_rng(1234 + N)
    t = np.arange(N)
    M = 2048 if N <= 8192 else 256
    ref = np.sin(2 * np.pi * 5 * t / N) + 0.05 * rng.standard_normal(N)
    rows = np.empty((M, N))
    q = M // 8
    rows[0 * q:1 * q] = rng.choice([-1.0, 1.0], size=(q, N))
    f0 = rng.uniform(0.0, 0.1, size=(q, 1))
    f1 = rng.uniform(0.2, 0.5, size=(q, 1))
    rows[1 * q:2 * q] = np.cos(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / N))
    spikes = 1e-3 * rng.standard_normal((q, N))
    spikes[np.arange(q), rng.integers(1, N, size=q)] += 1.0
    rows[2 * q:3 * q] = spikes
    out = rng.standard_normal((q, N))
    out[:, 0] += 7.5 * np.sqrt(N)                  # |mean d| = |x[0] - mean| ~ 7.5 sigma' ... (sigma includes the outlier)
    rows[3 * q:4 * q] = out
    odd = rng.standard_normal((2 * q, N)) + 0.5 * np.roll(ref, 7)
    sd = odd.std(axis=1, ddof=1, keepdims=True)
    rows[4 * q:6 * q] = odd / sd * np.sqrt(1.998 * 2.0 ** rng.choice([-21, -3, 1, 9, 41], size=(2 * q, 1)))
    rows[6 * q:7 * q] = np.sin(2 * np.pi * (t[None, :] + rng.integers(0, 64, size=(q, 1))) / 64.0) + 1e-3 * rng.standard_normal((q, N))
    rows[7 * q:] = rng.standard_normal((M - 7 * q, N)) + rng.uniform(-3, 3, size=(M - 7 * q, 1)) * np.roll(ref, -11)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
    assert_scores_match(lag, mv, olag, omv, gap, max_ties=max(2, M // 8))   # the fp64 kernels first (periodic rows tie)
    est, flags, E = db.screen_estimates(N)     # (MaxLag = N: no lag filter, so the pass's selection re-evaluates few rows)
    vouched = ((flags >> 31) & 1 == 0) & ((flags & (16 | 32)) == 0)
    assert vouched.sum() > M // 2                                            # the pass did vouch for most rows
    err = np.abs(np.abs(est[vouched]) - np.abs(mv[vouched]))
    worst = float(err.max() / E)
    print("N = %d: worst |estimate - exact| / E = %.3g over %d rows (E = %.3g)" % (N, worst, int(vouched.sum()), E))
    assert worst <= 1.0 / 8.0, (worst, E)
    db.close()


def test_screened_run_1m_rows_no_planted_copies(muse, eng, oracle):
    """BASELINE's 1 M x 4096 shape WITHOUT the planted copies of the reference (muse_hip.h,
    MUSE_SYNTH_NO_COPIES), so the top-N is a field of distinct scores instead of a thousand-way tie at 1.0 and a
    screening bug that dropped a candidate could not hide.  The screened Run's records are checked (a) against the
    oracle's Results over the GPU's own fp64 scores of all rows (membership, order, lags) and (b) row by row against
    the CPU oracle's scores of the returned rows (copied back byte-identical)."""
    M, N = 1_000_000, 4096
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x5EED, copies=False)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    assert np.sum(np.abs(np.abs(mv) - 1.0) < 1e-9) == 0                      # no copies indeed
    eng.set_screening(True)
    try:
        rng = np.random.default_rng(3)
        cases = [(None, 0, 15, 20, 0.0, 0, True), (None, 0, 4096, 100, 0.0, 0, True), (None, 0, 15, 20, 0.0, -1, False),
                 (None, 0, 100, 256, 0.05, 1, False)]
        gid = rng.integers(0, 20000, size=M).astype(np.int32)
        cases.append((gid, 20000, 15, 20, 0.0, 0, True))
        for args in cases:
            got = db.run(*args)
            assert db.last_run_path() == 1, args                             # the path under test ran
            scr, pairs = db.last_run_info()
            exp = oracle.results(lag, mv, args[0], args[1], args[6], args[2], args[3], args[4], args[5])
            assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist(), args
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
            assert len(set(np.round(got[2], 12).tolist())) > len(got[2]) // 2   # distinct scores, not a tie at the top
            if len(got[0]):
                back = np.concatenate([dg.read(int(i), 1) for i in got[0]])
                olag, omv, gap = oracle.batch_scores(ref, back)
                s = np.clip(np.abs(omv), None, 1.0) if args[6] else np.clip(omv, -1.0, 1.0)
                np.testing.assert_allclose(got[2], s, rtol=1e-9, atol=0)
                assert np.all((got[1] == olag) | (gap < 1e-12))
            print("no-copies Run %s: %d pairs re-evaluated (%.3f %% of the pairs, incl. the 1/1024 guard sample)"
                  % (str(args[1:]), pairs, 100.0 * pairs / (M / 2)))
    finally:
        eng.set_screening(False)
        db.close()


def test_screened_run_soak_1m_rows(muse, eng):
    """tools/screen_soak.py in the suite (5 trials): random filters / label groups on the 1 M synthetic rows, screened Run
    against the all-fp64 Run of the same batch."""
    M = 1_000_000
    dg, ref = muse.DeviceGroup.synthetic(eng, M, 4096, seed=2027)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    rng = np.random.default_rng(11)
    try:
        for trial in range(5):
            if trial % 3 == 2:
                G = int(rng.choice([100, 20000, 300000]))
                gid = rng.integers(0, G, size=M).astype(np.int32)
            else:
                gid, G = None, 0
            max_lag = int(rng.choice([0, 5, 15, 100, 2048, 4096]))
            top_n = int(rng.choice([1, 5, 20, 100, 256]))
            thr = float(rng.choice([0.0, 0.1, 0.4, 0.9]))
            sign = int(rng.choice([0, 1, -1]))
            absf = bool(rng.random() < 0.5)
            eng.set_screening(False)
            exp = db.run(gid, G, max_lag, top_n, thr, sign, absf)
            eng.set_screening(True)
            got = db.run(gid, G, max_lag, top_n, thr, sign, absf)
            key = (trial, G, max_lag, top_n, thr, sign, absf, db.last_run_path())
            assert len(got[0]) == len(exp[0]), key
            np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0, err_msg=str(key))
            rows = got[0]
            assert np.array_equal(lag[rows], got[1]), key
            exact = np.clip(np.abs(mv[rows]), None, 1.0) if absf else np.clip(mv[rows], -1.0, 1.0)
            np.testing.assert_allclose(got[2], exact, rtol=1e-12, atol=0, err_msg=str(key))
            assert len(rows) == 0 or np.all(np.abs(lag[rows]) <= max_lag), key
    finally:
        eng.set_screening(False)
        db.close()


@pytest.mark.parametrize("N", [4096, 3000, 512, 480, 1000, 2048, 1500, 5000, 8192, 16384, 10000])
def test_f32_storage_group_matches_oracle_on_rounded_rows(muse, eng, oracle, N):
    """SURVEY 8f-3, opt-in float32-STORAGE group: rows are rounded to float32 on the way in and widened exactly when the
    kernels consume them; arithmetic stays float64.  So the scores equal the oracle's on the ROUNDED rows (read back
    byte-identical through muse_group_read) to the usual 1e-6 / exact-lag bar -- incl. sigma == 0, NaN / Inf rows,
    pairs with sigmas far apart (hand-off kernel reading float32 rows too), an odd row count, appends in several
    pieces -- and differ from the float64 group's scores only by the input rounding."""
    rng = np.random.default_rng(909 + N)
    M = 515 if N <= 4096 else 131
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::4] += rng.uniform(-3, 3, size=(len(rows[::4]), 1)) * np.roll(ref, 5)
    rows[10, 5] = np.nan
    rows[12, :] = np.inf
    rows[20, :] = 3.5                       # sigma == 0
    rows[30] *= 1e20                        # partner of row 31: sigmas 1e20 apart -> rescaling kernel
    rows[41] *= 1e-25
    dg = muse.DeviceGroup(eng, N, 0, f32=True)
    dg.append(rows[:7])                     # one small piece, single rows, a slab
    for i in range(7, 20):
        dg.append(rows[i])
    dg.append(rows[20:])
    assert dg.M == M
    back = dg.read(0, M)
    assert np.array_equal(back, rows.astype(np.float32).astype(np.float64), equal_nan=True)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, back)
    assert math.isnan(mv[10]) and math.isnan(mv[12]) and mv[20] == 0.0 and lag[20] == 0
    assert_scores_match(lag, mv, olag, omv, gap)
    got = db.run(None, 0, 15, 10, 0.0, 0, True)
    exp = oracle.results(olag, omv, None, 0, True, 15, 10, 0.0, 0)
    assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist()
    np.testing.assert_allclose(got[2], exp[2], rtol=1e-9, atol=0)
    # against the float64 group: same lags on clear maxima, scores within the input rounding
    d64 = muse.DeviceBatch(eng, muse.DeviceGroup.from_rows(eng, rows), ref)
    lag64, mv64 = d64.scores()
    ok = ~np.isnan(mv64) & (gap > 1e-3)
    assert np.array_equal(lag[ok], lag64[ok])
    assert np.nanmax(np.abs(mv[ok] - mv64[ok])) < 1e-5
    with pytest.raises(muse.MuseError):
        muse.DeviceGroup(eng, 200, 0, f32=True)        # built for 257 .. 16384 only (FFT lengths 512 ... 16384)
    with pytest.raises(muse.MuseError):
        muse.DeviceGroup(eng, 20000, 0, f32=True)
    db.close()
    d64.close()


def test_f32_storage_group_synthetic_run(muse, eng, oracle):
    """the synthetic workload in a float32-storage group: every row against the oracle on the stored values, Run, the
    many-references entry point (one pass per reference on such a group) and the sharded Run."""
    M, N = 4000, 4096
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=77, copies=False, f32=True)
    db = muse.DeviceBatch(eng, dg, ref)
    rows = dg.read(0, M)
    lag, mv = db.scores()
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=8)
    assert_scores_match(lag, mv, olag, omv, gap, max_ties=1)
    ref2 = rows[17].copy()
    db2 = muse.DeviceBatch(eng, dg, ref2)
    both = muse.scores_many([db, db2])
    o2 = oracle.batch_scores(ref2, rows, nthreads=8)
    assert_scores_match(both[1][0], both[1][1], o2[0], o2[1], o2[2], max_ties=1)
    rec = db.run_shard(None, 0, 1000, 15, 5, 0.0, 0, True)
    exp = oracle.results(olag, omv, None, 0, True, 15, 5, 0.0, 0)
    assert (rec["series"] - 1000).tolist() == exp[0].tolist()
    db.close()
    db2.close()


def test_append_overlaps_a_running_score_pass(muse, eng, oracle):
    """muse_group_append uploads on the context's copy stream, so new rows can be sent while a score pass
    over the rows uploaded earlier is still running on the compute stream; the next pass is ordered behind the uploads
    (hipStreamWaitEvent) and sees every row.  Slab appends, per-Series appends through the staging pair, and a
    reallocation in between."""
    rng = np.random.default_rng(8086)
    N = 4096
    ref = rng.standard_normal(N)
    first = rng.standard_normal((3000, N)) + rng.uniform(-2, 2, size=(3000, 1)) * np.roll(ref, 4)
    more = rng.standard_normal((700, N)) + rng.uniform(-2, 2, size=(700, 1)) * np.roll(ref, -9)
    dg = muse.DeviceGroup(eng, N, 3200)                  # (capacity below the final size: one reallocation on the way)
    dg.append(first)
    db = muse.DeviceBatch(eng, dg, ref)
    db.score()                                           # asynchronous: the kernel is (or will be) running ...
    dg.append(more[:300])                                # ... while this slab goes up on the copy stream
    for r in more[300:340]:
        dg.append(r)                                     # per-Series appends (staging pair)
    db.score()                                           # second pass, again not waited for
    dg.append(more[340:])                                # grows the allocation: waits for both streams
    assert dg.M == 3700
    lag, mv = db.scores()
    rows = np.concatenate([first, more])
    assert np.array_equal(dg.read(0, 3700), rows)
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=8)
    assert_scores_match(lag, mv, olag, omv, gap)
    db.close()


def test_bench_two_ranks_rehearsal_on_one_gpu():
    """`python bench.py --gpus 2` without a launcher: the parent spawns two rank processes before touching the GPU, both ranks
    score their own shard (global row offsets), the per-shard records are gathered and merged, rank 0 prints ONE JSON line with
    n_gpus = 2 -- rehearsed here with both ranks on GPU 0 and the gather over gloo (RCCL refuses two ranks on one device; the
    RCCL path itself is covered at world size 1 above and by `--force-dist`)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["MASTER_PORT"] = "29641"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--rows", "20001", "--steps", "2", "--warmup", "1",
                        "--full", "--no-extras", "--with-config5", "--config5-rows", "3001", "--rehearse-on-one-gpu",
                        "--with-in-process-child", "--in-process-rows", "6000"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), r.stdout[-2000:]   # stdout = rank 0's ONE line, nothing else
    d = json.loads(r.stdout)
    assert d["n_gpus"] == 2 and d["rehearsal"] is True and d["dtype"] == "f64" and d["scaling"] == "weak"
    assert d["value"] > 0 and d["config"]["rows_per_gpu"] == 20001 and d["config"]["rows_total"] == 40002
    assert d["config"]["workload"].startswith("configs[3]-shaped") and "2 GPUs" in d["config"]["workload"]
    # the planted copy of the reference (synthetic row of rank 0) tops the merged list
    assert abs(d["top_score"] - 1.0) < 1e-9
    # what makes an N-rank line a measurement: every rank's own kernel time, device and PCI bus id; the roofline fraction is the
    # slowest rank's; the CPU baseline beside it at every N; no probe kernel inside the timed region
    assert [x["rank"] for x in d["ranks"]] == [0, 1]
    for x in d["ranks"]:
        assert x["kernel_ms_avg"] > 0 and x["launches_timed"] == 2 and x["rows"] == 20001
        assert x["pci_bus_id"].count(":") == 2 and "gfx950" in x["device"]
    assert d["distinct_devices"] == 1                      # (the rehearsal puts both ranks on GPU 0, and the line says so)
    rl = d["roofline"]
    kms = [x["kernel_ms_avg"] for x in d["ranks"]]
    assert rl["per_rank"]["kernel_ms_avg"]["max"] == max(kms) and rl["per_rank"]["kernel_ms_avg"]["min"] == min(kms)
    assert abs(rl["kernel_ms_avg"] - max(kms)) < 1e-12 and abs(rl["frac"] - rl["per_rank"]["frac"]["min"]) < 1e-12
    assert rl["per_gpu"] is True and rl["redo_ms_avg"] >= 0
    assert d["clock_probe_in_timed_region"] is False
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["cores"] >= 1 and cb["single_thread"]["value"] > 0
    # the one-process design a Go / C++ caller of the C ABI uses, measured by a CHILD of rank 0 once the ranks are done (at N ranks on
    # an N-GPU node: over those N devices; here both shards on GPU 0)
    ips = d["in_process_shards"]
    assert "error" not in ips, ips
    assert ips["devices"] == [0, 0] and ips["rows_per_shard"] == 6000 and ips["records_identical_to_one_context"] is True
    assert ips["value"] > 0 and "child process" in ips["note"]
    # BASELINE configs[4] at N ranks: seven lengths, every Group sharded over both ranks with its label groups on both, one shared Results
    c5, legs = d["config5_mixed_run"], d["config5_lengths"]
    assert c5["n_gpus"] == 2 and c5["lengths"] == [512, 1000, 4096, 5000, 16384, 20000, 65536] and c5["value"] > 0
    assert c5["shared_results"]["fetched"] == 20 and len(c5["shared_results"]["lengths_in_top_n"]) >= 2
    for e in legs:
        assert "error" not in e, e
        assert e["rows_total"] == 2 * e["rows"] and e["label_groups"] == e["rows_total"] // 50
        assert abs(e["kernel_ms_avg"] - e["kernel_ms_per_rank"]["max"]) < 1e-9 and e["kernel_ms_avg"] > 0 and e["run_ms"] > 0
        assert e["exchange"].startswith("all_gather")


def test_bench_plain_run_times_the_steps_and_dumps_the_last_records(eng, muse, tmp_path):
    """`python bench.py` without --full: the headline fields only, exactly --steps timed Runs, and --dump-outputs writes the
    records of the last one -- the same records a Run over the same seeded synthetic rows returns in this process"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    M, N, d = 20001, 4096, tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--rows", str(M), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), r.stdout[-2000:]
    line = json.loads(r.stdout)
    assert line["steps"] == 3 and line["ranks"][0]["launches_timed"] == 3 and line["ms_per_step"] > 0
    assert line["dtype"] == "f64" and line["unit"] == "series-pairs/s" and line["higher_is_better"] is True and line["value"] > 0
    for extra in ("cpu_baseline", "filter_and_refine_run", "f32_storage_group", "many_references", "two_sided_xcorr",
                  "in_process_shards", "long_series", "config5_mixed_run", "reference_bench_shapes"):
        assert extra not in line, extra
    got = {k: np.load(d / (k + ".npy")) for k in ("top_series", "top_lag", "top_score", "mean_abs_score")}
    assert all(a.dtype == np.float64 for a in got.values())
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    series, lag, score, mean_abs = db.run(None, 0, 15, 20, 0.0, 0, True)
    db.close()
    dg.close()
    assert len(series) == 20 and np.array_equal(got["top_series"], series) and np.array_equal(got["top_lag"], lag)
    assert np.array_equal(got["top_score"], score) and got["mean_abs_score"].shape == (1,)
    assert abs(got["mean_abs_score"][0] - mean_abs) <= 1e-12 * abs(mean_abs)
    assert line["top_score"] == score[0] and abs(score[0] - 1.0) < 1e-9    # (the planted copy of the reference)


def test_reference_bench_shapes_harness(muse):
    """go-muse_amd/host/muse_ref_bench.cpp (the reference's six `go test -bench` bodies over the C++ mirror; bench.py's
    reference_bench_shapes runs it as a child process): builds, runs, prints one JSON object with every benchmark and a positive
    time per op beside the README's figure."""
    import json
    import subprocess
    exe = muse.build.build_ref_bench()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    d = json.loads(r.stdout)
    assert sorted(d) == ["BenchmarkMuseBatchRun", "BenchmarkMuseBatchRunLarge", "BenchmarkMuseRun", "BenchmarkMuseRunLarge",
                         "BenchmarkXCorr", "BenchmarkXCorrWithX"]
    for name, o in d.items():
        assert o["ns_per_op"] > 0 and o["reps"] >= 3 and "source" in o, name
    assert d["BenchmarkMuseRun"]["readme_ns_per_op"] == 5019 and d["BenchmarkXCorrWithX"]["readme_ns_per_op"] == 4910405
    assert d["BenchmarkMuseRunLarge"]["ns_per_op"] < 128044546 / 10      # (two orders below the README's laptop on any MI355X box)


def test_many_references_on_a_float32_storage_group(muse, eng, oracle):
    """muse_batch_score_many over an opt-in float32-storage group at n = 4096 (N = 4096 and a padded length): one pass over the
    float32 rows for all references; per reference the scores of the oracle on the ROUNDED rows, and what single passes give"""
    for N in (4096, 3500):
        rng = np.random.default_rng(4242 + N)
        M, R = 301, 3
        rows = rng.standard_normal((M, N))
        refs = [rng.standard_normal(N) for _ in range(R)]
        rows[::3] += 2.0 * np.roll(refs[1], 11)
        rows[7, 3] = np.nan
        rows[9] = -2.0
        dg = muse.DeviceGroup.from_rows(eng, rows, f32=True)
        back = dg.read(0, M)
        bs = [muse.DeviceBatch(eng, dg, r) for r in refs]
        out = muse.scores_many(bs)
        for r in range(R):
            olag, omv, gap = oracle.batch_scores(refs[r], back)
            assert_scores_match(out[r][0], out[r][1], olag, omv, gap)
            lag1, mv1 = bs[r].scores()
            assert np.array_equal(lag1, out[r][0]) and np.allclose(mv1, out[r][1], rtol=1e-12, atol=1e-15, equal_nan=True)
        for b in bs:
            b.close()
        dg.close()


# ------------------------------------------------ batched two-sided xCorr (xcorr.go:102-153)
def _oracle_xcorr_rows(oracle, X, Y, n, normalize):
    """oracle.xcorr per pair: cc rows (None where nil), lags, values and the top-two |cc| gap of each pair"""
    ccs, lags, mvs, gaps = [], [], [], []
    for x, y in zip(X, Y):
        cc, lag, mv = oracle.xcorr(x, y, n, normalize)
        ccs.append(cc)
        lags.append(lag)
        mvs.append(mv)
        if cc is None or not np.all(np.isfinite(cc)):
            gaps.append(1.0)
        else:
            a = np.sort(np.abs(cc))[::-1]
            gaps.append((a[0] - a[1]) / a[0] if a[0] > 0 else 0.0)
    return ccs, np.array(lags), np.array(mvs), np.array(gaps)


def _check_xcorr_batch(eng, oracle, X, Y, n, normalize):
    cc, lag, mv, nil = eng.xcorr_batch(X, Y, n, normalize, want_cc=True)
    occ, olag, omv, gap = _oracle_xcorr_rows(oracle, X, Y, n, normalize)
    onil = np.array([c is None for c in occ])
    assert np.array_equal(nil.astype(bool), onil)          # (nil, 0, 0): xcorr.go:110-127
    assert np.all(lag[onil] == 0) and np.all(mv[onil] == 0.0)
    live = ~onil
    # (a constant series that is NOT normalized correlates to the same value at every lag: an exact tie by construction)
    worst = assert_scores_match(lag[live], mv[live], olag[live], omv[live], gap[live], max_ties=0 if normalize else 2)
    for i in np.nonzero(live)[0]:
        if np.all(np.isfinite(occ[i])):
            scale = max(np.max(np.abs(occ[i])), 1e-300)
            assert np.max(np.abs(cc[i] - occ[i])) <= 1e-9 * scale + 1e-12, (i, n, normalize)
        else:
            assert np.all(np.isnan(cc[i]))
    # the outputs-only form returns the same lags and values
    lag2, mv2, nil2 = eng.xcorr_batch(X, Y, n, normalize)
    assert np.array_equal(lag2, lag) and np.array_equal(nil2, nil)
    assert np.array_equal(np.isnan(mv2), np.isnan(mv)) and np.array_equal(mv2[~np.isnan(mv)], mv[~np.isnan(mv)])
    return worst


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384, 32768, 65536])
@pytest.mark.parametrize("normalize", [True, False])
def test_xcorr_batch_matches_oracle(eng, oracle, n, normalize):
    rng = np.random.default_rng(n + int(normalize))
    M = 11 if n <= 8192 else 7
    for N in (n, n - n // 4 - 3):                          # no padding (circular) and leading zero pads
        X = rng.normal(size=(M, N)) * rng.uniform(0.1, 30.0, size=(M, 1)) + rng.normal(size=(M, 1)) * 5.0
        Y = rng.normal(size=(M, N)) * rng.uniform(0.1, 30.0, size=(M, 1)) - 2.0
        Y[1] = np.roll(X[1], 7) * -3.0 + 1.0               # a strong negative peak at a known lag
        X[2] = 4.25                                        # sigma(x) == 0: nil when normalized, zero-lag ... product otherwise
        Y[3] = -1.5                                        # sigma(y) == 0
        X[4] *= 1e9                                        # scales far apart inside one pair
        Y[4] *= 1e-7
        if N == n:
            Y[0, N // 3] = np.nan                          # every cc NaN: lag 0, mv NaN
        # finite samples whose SQUARES leave the float64 range (xcorr.go:108-143 still returns numbers): raw -- finite cc of
        # magnitude 1e200; normalized -- gonum's sigma is +Inf and the series all zeros (1e160), or (sum d)^2 overflows too and
        # everything is NaN (1e200)
        X[5] *= 1e200
        Y[6] *= 1e160
        _check_xcorr_batch(eng, oracle, X, Y, n, normalize)


@pytest.mark.parametrize("n", [8192, 16384])
def test_xcorr_batch_real_and_pair_packed_kernels(eng, oracle, n):
    """n = 8192, 16384: automatic selection transforms each series as a REAL series on the 4096- / 8192-point machinery
    (xcorr_two_sided_real8k / real16k); test hook 12 keeps the pair-packed kernels (xcorr_two_sided_small<13 / 14>).  Both against
    the oracle, padded and not, series shorter than one request row, more pairs than one resident set of workgroups."""
    rng = np.random.default_rng(n)
    M = 19 if n == 16384 else 2100
    for lens in ((n, n), (n - n // 4 - 3, n), (n // 2 + 808, 3 * n // 4 - 287), (n, 37)):
        if M > 100 and lens != (n, n):
            M = 23
        X = rng.normal(size=(M, lens[0])) * rng.uniform(0.1, 30.0, size=(M, 1)) + 2.0
        Y = rng.normal(size=(M, lens[1])) * 4.0 - 1.0
        k = min(lens)
        Y[1, :k] = X[1, :k] * -2.0
        X[2] = 1.25
        Y[3, 17] = np.nan
        for variant in (0, 12):
            eng.set_kernel(variant)
            try:
                for normalize in (True, False):
                    _check_xcorr_batch(eng, oracle, X, Y, n, normalize)
            finally:
                eng.set_kernel(0)


@pytest.mark.parametrize("n", [32768, 65536])
def test_xcorr_batch_long_series_single_read_and_its_redo_list(eng, oracle, n):
    """n >= 32768 with N = n reads the rows once and squares the spectrum UNSCALED; pairs whose series differ by more than 2^16 in
    sigma, or whose magnitudes are extreme (variance exponents beyond +-400: the square would leave the float64 range), are listed
    and redone by the launch that takes the statistics first and scales by exact powers of two.  Every kind of pair in one batch,
    more listed pairs than one workgroup takes, against the oracle (full cc vectors)."""
    rng = np.random.default_rng(n)
    M = 11
    X = rng.normal(size=(M, n)) * 3.0 + 1.0
    Y = rng.normal(size=(M, n)) - 0.5
    X[8] = 0.0                                             # an all-zero series beside one of magnitude 1e150: listed (raw: the
    Y[8] *= 1e150                                          # unscaled square of y alone would overflow), nil when normalized
    X[9] *= 1e-170                                         # squares underflow to zero beside 1e148: listed
    Y[9] *= 1e148
    Y[0] = np.roll(X[0], -11) * 2.0                        # an ordinary pair with a clear peak
    X[1] *= 1e130; Y[1] *= 1e130                           # extreme magnitudes, equal scale: listed
    X[2] *= 1e-130; Y[2] *= 1e-130                         # tiny magnitudes: listed
    X[3] *= 1e12                                           # scales 10^12 apart: listed
    Y[4] *= 1e-9                                           # listed
    X[5] = -7.0                                            # sigma(x) == 0
    Y[6, 5] = np.inf                                       # every cc NaN
    X[7] *= 3e4                                            # 2^15 apart in sigma: NOT listed (inside the spread the square tolerates)
    for normalize in (True, False):
        _check_xcorr_batch(eng, oracle, X, Y, n, normalize)


@pytest.mark.parametrize("n", [4096, 32768])
def test_xcorr_batch_raw_products_up_to_the_float64_range(eng, oracle, n):
    """Raw xCorr of finite samples whose product is huge: the reference (xcorr.go:108-143) returns numbers as long as
    n max|x| max|y| stays inside the float64 range and NaN beyond.  Round 5 returned NaN from 2^974 / n^2 on (a bound on the
    recomputation's intermediates: ADVICE r05); now the pair is recomputed at magnitude 1 and scaled back exactly, so the
    boundary is the reference's: 2^520 x 2^460 (cc ~ 2^990) is finite and equal to the oracle's, 2^520 x 2^500 is NaN in both."""
    rng = np.random.default_rng(n + 9)
    M = 6
    X = rng.normal(size=(M, n))
    Y = rng.normal(size=(M, n))
    Y[0] = np.roll(X[0], 5) * 1.5
    X[0] *= 2.0 ** 520; Y[0] *= 2.0 ** 460           # finite in the reference: cc up to ~ n 2^980
    X[1] *= 2.0 ** 500; Y[1] *= 2.0 ** 495           # ~ n 2^995 (+ a few binades of the sum): still finite
    X[2] *= 2.0 ** 520; Y[2] *= 2.0 ** 500           # n 2^1020 > 2^1024: the reference's products overflow
    X[3] *= 2.0 ** 1000; Y[3] *= 2.0 ** -1000        # magnitudes cancel: an ordinary result
    X[4] *= 2.0 ** -400; Y[4] *= 2.0 ** -400         # tiny products (2^-800): recomputed at magnitude 1, scaled back
    _check_xcorr_batch(eng, oracle, X, Y, n, False)


def test_xcorr_batch_different_lengths_and_raised_n(eng, oracle):
    rng = np.random.default_rng(77)
    M = 9
    X = rng.normal(size=(M, 700))
    Y = rng.normal(size=(M, 1000)) + np.linspace(0.0, 3.0, 1000)
    for normalize in (True, False):
        _check_xcorr_batch(eng, oracle, X, Y, 1024, normalize)     # each series padded on its own (xcorr.go:129-130)
        _check_xcorr_batch(eng, oracle, X, Y, 600, normalize)      # n raised to max(n, lenx, leny) = 1000: the direct kernel
    # the bench workload's shape through the resident-groups entry point
    muse = pkg()
    gx = muse.DeviceGroup.from_rows(eng, X[:, :512])
    gy = muse.DeviceGroup.from_rows(eng, Y[:, :512])
    lag, mv, nil = muse.xcorr_groups(gx, gy, 512, True)
    _, olag, omv, gap = _oracle_xcorr_rows(oracle, X[:, :512], Y[:, :512], 512, True)
    assert_scores_match(lag, mv, olag, omv, gap)
    with pytest.raises(muse.MuseError):
        muse.xcorr_groups(gx, muse.DeviceGroup.from_rows(eng, Y[:3, :512]), 512, True)   # row counts differ


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384, 32768, 65536])
@pytest.mark.parametrize("geom", ["short_long", "full_tiny", "two_full", "minus_one", "full_full"])
def test_xcorr_batch_pad_geometries(eng, oracle, n, geom):
    """every batched length runs on the xCorrWithX transforms (x read backwards, the spectrum squared; n >= 32768: on the
    long-series kernel's four-step transform): every pad geometry, each series padded on its own (xcorr.go:129-130)"""
    lens = {"short_long": (n // 6 + 17, 3 * n // 4 - 1), "full_tiny": (n, 10), "two_full": (2, n), "minus_one": (n - 1, n),
            "full_full": (n, n)}[geom]
    rng = np.random.default_rng(lens[0] * 7 + lens[1])
    M = 13 if n <= 4096 else 5
    X = rng.normal(size=(M, lens[0])) * rng.uniform(0.5, 4.0, size=(M, 1)) + 3.0
    Y = rng.normal(size=(M, lens[1])) - np.linspace(0.0, 1.0, lens[1])
    k = min(lens)
    Y[3, :k] = X[3, :k][::-1] * 2.0                         # a mirrored copy: the peak of a convolution, not of the correlation
    Y[4, :k] = -X[4, :k]
    for normalize in (True, False):
        _check_xcorr_batch(eng, oracle, X, Y, n, normalize)


@pytest.mark.parametrize("M", [1, 2, 3, 257])
def test_xcorr_batch_few_and_many_pairs(eng, oracle, M):
    """pair counts below one workgroup's share (n = 512: eight pairs per workgroup iteration), odd counts, more pairs than one
    resident set of sub-groups handles at once"""
    rng = np.random.default_rng(M)
    for n in (512, 1024, 4096):
        X = rng.normal(size=(M, n - 7))
        Y = rng.normal(size=(M, n)) * 3.0 + 1.0
        _check_xcorr_batch(eng, oracle, X, Y, n, True)


def test_xcorr_batch_golden_tables(eng, golden):           # xcorr_test.go:86-202 through the batch entry (n = 5: pair by pair)
    for c in golden["xcorr"]["cases"]:
        cc, lag, mv, nil = eng.xcorr_batch([c["x"]], [c["y"]], len(c["x"]), c["normalize"], want_cc=True)
        if c["cc"] is None:
            assert nil[0] == 1 and lag[0] == 0 and mv[0] == 0.0
        else:
            assert nil[0] == 0
            assert np.max(np.abs(cc[0] - np.array(c["cc"], float))) <= golden["xcorr"]["tol"]
            assert lag[0] == c["idx"]
            _check_sign(mv[0], c["sign"])


def test_xcorr_batch_many_pairs_4096(eng, oracle):
    """2 000 pairs of rect + noise series (the bench's extra object at a size the oracle still finishes)"""
    rng = np.random.default_rng(5)
    M, N = 2000, 4096
    t = np.arange(N)
    c = rng.integers(N // 4, 3 * N // 4, size=(M, 1))
    X = (np.abs(t - c) <= 5) * 1.5 + 0.1 * rng.normal(size=(M, N))
    Y = (np.abs(t - c - rng.integers(-40, 40, size=(M, 1))) <= 8) * rng.uniform(-3, 3, size=(M, 1)) + 0.1 * rng.normal(size=(M, N))
    lag, mv, nil = eng.xcorr_batch(X, Y, N, True)
    sel = rng.choice(M, 150, replace=False)
    _, olag, omv, gap = _oracle_xcorr_rows(oracle, X[sel], Y[sel], N, True)
    assert not nil.any()
    assert_scores_match(lag[sel], mv[sel], olag, omv, gap)


# ------------------------------------------------ one process, several devices behind Batch.Run
def _mirror_group(muse, rows, graphs, hosts):
    g = muse.NewGroup("targets")
    g.Add(*[muse.NewSeries(rows[i], muse.NewLabels({"graph": "g%d" % graphs[i], "host": "h%d" % hosts[i]}))
            for i in range(len(rows))])
    return g


def _fetch(batch):
    scores, mean = batch.Results.Fetch()
    return [(s.Labels.ID(), s.Lag, s.PercentScore) for s in scores], mean


def test_batch_run_sharded_over_engine_list(muse, eng, oracle):
    """NewBatch(..., engines=[...]).Run shards the Comparison group over the listed contexts (here: device 0 three times,
    plus every device the box has) and must return exactly the one-device Run's Scores -- for Run(nil) (per-shard top-N),
    for label groups that straddle every shard (per-group maxima merged before filtering) and under filters; the
    one-device scores themselves are checked against the oracle's Results."""
    rng = np.random.default_rng(31)
    M, N = 2001, 4096
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::7] += 1.5 * np.roll(ref, 5)[None, :]
    rows[3::11] -= 2.5 * np.roll(ref, -9)[None, :]
    rows[4] = 1.25                                         # sigma == 0
    rows[6, 100] = np.nan                                  # first member of graph 6: that group never passes
    rows[6 + 50 * 13, 7] = np.nan                          # a later member of graph 6 + ... in another shard
    graphs = np.arange(M) % 50                             # every graph has members in every shard
    hosts = np.arange(M) // 50
    ndev = muse.device_count()
    lists = [[0, 0, 0], [0, 0], list(range(ndev)) * (1 if ndev > 1 else 4)]
    cases = [(None, N, 20, 0.0, 0), (["graph"], N, 20, 0.0, 0), (["host"], N, 9, 0.0, 0),
             (["graph"], 6, 10, 0.02, 1), (["graph", "host"], N, 300, 0.0, 0)]
    refs = muse.NewSeries(ref, muse.NewLabels({"graph": "ref"}))
    one_group = _mirror_group(muse, rows, graphs, hosts)
    expect = []
    for by, max_lag, top, thr, sf in cases:
        b = muse.NewBatch(refs, one_group, muse.NewResults(max_lag, top, thr, sf), 8, engine=eng)
        b.Run(by)
        expect.append(_fetch(b))
    # anchor: the grouped one-device Run against the oracle's Results over oracle scores
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=16)
    oi, ol, osc, omean = oracle.results(olag, omv, graphs.astype(np.int32), 50, True, N, 20, 0.0, 0)
    got = expect[1][0]
    assert [g[1] for g in got] == list(ol)
    assert np.allclose([g[2] for g in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    for devs in lists:
        engines = [muse.Engine(d) for d in devs]
        grp = _mirror_group(muse, rows, graphs, hosts)
        for limit in (muse.muse.EXACT_FEED_MAX_GROUPS, 0):   # the reference's feed, and the pre-selecting paths of very large Runs
            saved, muse.muse.EXACT_FEED_MAX_GROUPS = muse.muse.EXACT_FEED_MAX_GROUPS, limit
            try:
                for c, (by, max_lag, top, thr, sf) in enumerate(cases):
                    b = muse.NewBatch(refs, grp, muse.NewResults(max_lag, top, thr, sf), 8, engines=engines)
                    b.Run(by)
                    got, mean = _fetch(b)
                    assert got == expect[c][0], (devs, c, limit)
                    assert mean == expect[c][1] or (math.isnan(mean) and math.isnan(expect[c][1]))
            finally:
                muse.muse.EXACT_FEED_MAX_GROUPS = saved
    # fewer rows than devices (empty shards) and the reference's own table over three shards
    tiny = _mirror_group(muse, rows[:3], graphs[:3], hosts[:3])
    b1 = muse.NewBatch(refs, tiny, muse.NewResults(N, 5, 0.0, 0), 1, engine=eng)
    b3 = muse.NewBatch(refs, _mirror_group(muse, rows[:3], graphs[:3], hosts[:3]), muse.NewResults(N, 5, 0.0, 0), 1,
                       engines=[muse.Engine(0) for _ in range(5)])
    b1.Run(None)
    b3.Run(None)
    assert _fetch(b1) == _fetch(b3)


# ------------------------------------------------ device unit test: the argmax step of the n = 4096 kernels
def _wave_argmax_expected(cc, wave):
    """maxAbsIndex (xcorr.go:39-50) over the lag indices a wave owns (t + 256 m, t in the wave's 64 lanes): the first index
    whose |value| is the largest, only values above 0 count."""
    idx = (np.arange(64)[None, :] + 64 * wave + 256 * np.arange(16)[:, None]).ravel()
    idx.sort()
    a = np.abs(cc[idx])
    if not (a.max() > 0):
        return 0.0, cc[64 * wave], 2147483647
    k = int(idx[np.argmax(a)])  # argmax returns the first maximum of the ascending indices
    return float(a.max()), float(cc[k]), k


def test_wave_argmax_tie_rules(eng):                   # foldk_device.h wave_argmax_store
    rng = np.random.default_rng(77)
    cases = []
    base = rng.standard_normal((2, 4096))
    cases.append(base.copy())                              # no ties
    c = base.copy()                                        # the same maximum in several registers of one lane, both signs
    c[0, [5 + 256 * 9, 5 + 256 * 3, 5 + 256 * 12]] = [7.5, -7.5, 7.5]
    c[1, [200 + 256 * 15, 200]] = [-9.25, 9.25]
    cases.append(c)
    c = base.copy()                                        # the same maximum in several lanes of a wave and in several waves
    c[0, [70 + 256 * 4, 100 + 256 * 2, 127 + 256 * 2, 3 + 256 * 2, 250 + 256]] = [8.0, -8.0, 8.0, 8.0, -8.0]
    c[1, [64 * w + 63 + 256 * 15 for w in range(4)]] = 6.0
    c[1, 64 + 256 * 15] = -6.0
    cases.append(c)
    c = np.zeros((2, 4096))                                # nothing above 0 / a single non-zero value in the last place
    c[1, 4095] = -1e-300
    cases.append(c)
    c = np.full((2, 4096), 3.0)                            # every value ties
    c[1] = -3.0
    cases.append(c)
    c = base.copy()                                        # maxima that differ in the last bit only (low word decides)
    c[0, 1000] = 11.0
    c[0, 17] = np.nextafter(11.0, 12.0)
    c[0, 3000] = -np.nextafter(11.0, 12.0)
    c[1, 2047] = -np.nextafter(11.0, 0.0)
    c[1, 2048] = 11.0
    cases.append(c)
    c = base.copy()                                        # denormals and huge values
    c[0] *= 1e-310
    c[1] *= 1e300
    cases.append(c)
    for ci, c in enumerate(cases):
        out = eng.wave_argmax(c[0], c[1])
        for w in range(4):
            for s in range(2):
                m, sv, k = _wave_argmax_expected(c[s], w)
                got = out[w, s]
                assert got[0] == m and int(got[2]) == k, (ci, w, s, got, (m, sv, k))
                if k != 2147483647 or w == 0:              # (nothing above 0: the kernels only use wave 0's cc[0])
                    assert got[1] == sv, (ci, w, s, got, (m, sv, k))
