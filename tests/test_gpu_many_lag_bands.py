"""GPU tests of the many-references lag bands (muse_batch_score_many_in_lag_bands / _run_many_in_lag_bands, run with -m gpu on an
MI355X): R references against one resident group, EACH inside its own lag range or band and under its own sign, from one read of
the rows -- the references' table rows packed into the tiles of one fp64 matrix product whose descriptors are per reference
(xcorr_window_many_each_mfma), the uniform packed kernels where a launch's members ask one question, the single-reference kernel for
a reference alone in its launch, and a reference's own single pass where it is not on the direct product.

Expected values never come from the code under test: per reference and series, the definition in include/muse_hip.h applied in
numpy (tests/_lagband.py) to the correlation slice the CPU oracle returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are tests/test_gpu_lag_band.py's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact on EVERY row:
tests/test_many_lag_bands_cpu.py checks on the same tuples (tests/_manylagbands.py) that the oracle flags no tie.  Every batch must
also be BIT-IDENTICAL to its own scores_in_lag_band(lo_r, hi_r, sign_r), in both orders of the two calls, and to a repeat."""
import ctypes

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LSW
import _manylagbands as MB
import _manylagrange as MLR
from _load import pkg
from test_gpu_lag_band import _assert_run, _same_selection, check
from test_gpu_many_lag_band import batches, close, refused, same_bits, state

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


def wants(muse, N, n, assign):
    """per member what the planner says of a list that does not share one question: ("each" | "uniform" | "alone", tiles)"""
    bands, signs = MB.bands_of(assign), MB.signs_of(assign)
    p = muse.many_lag_bands_plan(N, False, bands, signs)
    out = []
    for r in range(len(assign)):
        l = int(p["launch_of"][r])
        assert l >= 0 and p["path"][r] == muse.binding.MUSE_IN_WINDOW_MFMA
        mem = [q for q in range(len(assign)) if p["launch_of"][q] == l]
        asked = {(LB.clip(n, *bands[q]), signs[q]) for q in mem}
        out.append(("alone" if len(mem) == 1 else "uniform" if len(asked) == 1 else "each", int(p["tiles_of"][l])))
    return out


def check_name(muse, name, path, want, clipped, sign, single_name, tag):
    kind, tiles = want
    if kind == "each":
        assert name.startswith("xcorr_window_many_each_mfma<%d, " % tiles) and path == 0, (tag, name, path)
    elif kind == "uniform":
        head = "xcorr_window_many_mfma<" if sign == 0 and clipped[0] <= 0 <= clipped[1] else "xcorr_window_many_signed_mfma<"
        assert name.startswith("%s%d, " % (head, tiles)) and path == 0, (tag, name, path)
    else:                                                            # alone in its launch: named as the single call names it
        assert path == muse.binding.MUSE_IN_WINDOW_MFMA and name == single_name and name.startswith("xcorr_window_"), (tag, name, single_name)


def run_lists(muse, eng, oracle, N, lists, m=MB.M):
    """every list against the definition, bit for bit against each batch's own single call (both orders) and a repeat, named as
    the planner says; returns (members of mixed launches, rows with nothing)"""
    B = muse.binding
    ref, rows, refs = MB.case(N)
    exp, n = MB.expectations(oracle, N)
    dg = muse.DeviceGroup.from_rows(eng, rows[:m])
    dbs = batches(muse, eng, dg, refs)
    twins = batches(muse, eng, dg, refs)
    assert dbs[0].n == n
    for db in dbs:
        db.scores()
    each = none = 0
    for k, (tag0, idx, assign) in enumerate(lists):
        sel = [dbs[r] for r in idx]
        bands, signs = MB.bands_of(assign), MB.signs_of(assign)
        clipped = [LB.clip(n, lo, hi) for lo, hi in bands]
        if any(c is None for c in clipped):                          # (FAR at n = 128: nothing of a band is left)
            refused(muse, eng, sel, lambda: muse.score_many_in_lag_bands(sel, bands, signs), B.MUSE_ERR_INVALID)
            continue
        uniform = len(set(assign)) == 1
        want = None if uniform else wants(muse, N, n, assign)
        first_alone = k % 2 == 1                                     # both orders of the two forms
        single = single_names = None
        if first_alone:
            single = [db.scores_in_lag_band(lo, hi, s) for db, (lo, hi), s in zip(sel, bands, signs)]
            single_names = [eng.kernel_name(db) for db in sel]
        got = muse.scores_many_in_lag_bands(sel, bands, signs)
        names = [eng.kernel_name(db) for db in sel]
        paths = [db.last_in_window_path() for db in sel]
        again = muse.scores_many_in_lag_bands(sel, bands, signs)
        assert names == [eng.kernel_name(db) for db in sel]
        if single is None:
            single = [db.scores_in_lag_band(lo, hi, s) for db, (lo, hi), s in zip(sel, bands, signs)]
            single_names = [eng.kernel_name(db) for db in sel]
        if uniform:                                                  # the bits and the kernel names of scores_many_in_lag_band
            tw = [twins[r] for r in idx]
            ugot = muse.scores_many_in_lag_band(tw, bands[0][0], bands[0][1], signs[0])
            assert names == [eng.kernel_name(t) for t in tw] and paths == [t.last_in_window_path() for t in tw], (tag0, names)
            assert all(same_bits(a, b) for a, b in zip(got, ugot)), tag0
        for j, r in enumerate(idx):
            (lo, hi), s = bands[j], signs[j]
            tag = "%s N=%d M=%d ref=%d [%d, %d] sign %+d" % (tag0, N, m, r, lo, hi, s)
            e = exp[(r, lo, hi, s)]
            none += check(got[j][0], got[j][1], (e[0][:m], e[1][:m], e[2][:m]), n, (lo, hi), s, tag)
            assert same_bits(got[j], single[j]) and same_bits(got[j], again[j]), tag
            assert sel[j].lag_window() == -1 and sel[j].last_run_path() == 0, tag
            if want:
                check_name(muse, names[j], paths[j], want[j], clipped[j], s, single_names[j], tag)
                each += want[j][0] == "each"
    close(dbs, twins, dg)
    return each, none


# ------------------------------------------------------------------ 1. every assignment, permuted and cut
@pytest.mark.parametrize("N", MB.DIRECT_NS)
def test_every_list_is_the_single_calls(muse, eng, oracle, N):
    """MIXED, SYMMETRIC, CUT, ALONE, FAR and UNIFORM, reversed, rotated against the references and cut to R = 2 and 3: N below one
    chunk, an odd row length (the 8-byte loads), a short last chunk"""
    each, none = run_lists(muse, eng, oracle, N, MB.all_lists())
    assert each >= 40 and none >= 4, (each, none)                    # (members of mixed launches; the constant row, rows with no value of the sign)


@pytest.mark.parametrize("m", MB.SMALL_MS)
def test_row_counts(muse, eng, oracle, m):
    """M = 1, 15 and 17: the tail rows of a workgroup"""
    lists = [l for name, assign in MB.ASSIGNMENTS[:4] for l in MB.lists(name, assign)[:2]]
    each, _ = run_lists(muse, eng, oracle, MB.SMALL_M_N, lists, m)
    assert each >= 20


# ------------------------------------------------------------------ 2. a reference that is not on the direct product
def test_one_reference_off_the_direct_product(muse, eng, oracle):
    """N = 480: MIXED's first three with a reference at 200 lags between them (the masked transform pass at FFT length 512) -- the
    packed ones keep their bits and their mixed launch, the other equals its single call; the same list on a float32-storage group:
    every reference takes its single pass; and at N = 5000, where 200 lags are not built, the whole call is refused with the single
    call's status and nothing changed"""
    B = muse.binding
    N = 480
    ref, rows, refs = MB.case(N)
    assert (N, 1) == (MB.WIDE_N, MB.WIDE_REF)
    assign = [MB.MIXED[0], MB.WIDE, MB.MIXED[1], MB.MIXED[2]]
    bands, signs = MB.bands_of(assign), MB.signs_of(assign)
    p = muse.many_lag_bands_plan(N, False, bands, signs)
    assert list(p["launch_of"]) == [0, -1, 0, 0] and list(p["path"]) == [2, 3, 2, 2] and p["launches"] == 1
    wide_exp, n = LB.expect(oracle, refs[1], rows, ((1, 200),), (1,))
    for f32 in (False, True):
        with np.errstate(over="ignore"):                             # (the Inf row of the case)
            rws = rows.astype(np.float32).astype(np.float64) if f32 else rows
        dg = muse.DeviceGroup.from_rows(eng, rws, f32=f32)
        dbs, un = batches(muse, eng, dg, refs[:4]), batches(muse, eng, dg, refs[:4])
        got = muse.scores_many_in_lag_bands(dbs, bands, signs)
        names = [eng.kernel_name(db) for db in dbs]
        for r in range(4):
            (lo, hi), s = assign[r]
            one = un[r].scores_in_lag_band(lo, hi, s)
            tag = "off the product f32=%d ref=%d [%d, %d] sign %+d" % (f32, r, lo, hi, s)
            assert same_bits(got[r], one), tag
            assert dbs[r].lag_window() == -1
            if f32 or r == 1:                                        # its own single pass: the single call's kernel and path
                assert names[r] == eng.kernel_name(un[r]) and dbs[r].last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, (tag, names[r])
            else:
                assert names[r].startswith("xcorr_window_many_each_mfma<2, ") and dbs[r].last_in_window_path() == 0, (tag, names[r])
        if not f32:
            check(got[1][0], got[1][1], wide_exp[(1, 200, 1)], n, (1, 200), 1, "the 200-lag reference")
        close(dbs, un, dg)
    rng = np.random.default_rng(5)
    dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((6, 5000)))
    dbs = [muse.DeviceBatch(eng, dg, rng.standard_normal(5000)) for _ in range(4)]
    muse.score_many_in_lag_bands(dbs, bands[:1] + bands[2:] + [(1, 9)], 0)   # (a mixed packed pass's scores to leave alone)
    assert eng.kernel_name(dbs[0]).startswith("xcorr_window_many_each_mfma<")
    with pytest.raises(muse.MuseError) as e:
        dbs[1].scores_in_lag_band(1, 200, 1)
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, bands, signs), e.value.status)
    assert e.value.status == B.MUSE_ERR_UNSUPPORTED
    close(dbs, dg)


# ------------------------------------------------------------------ 3. refusals against a snapshot
def test_refusals_leave_everything_as_it_was(muse, eng):
    B = muse.binding
    L = B.load()
    rng = np.random.default_rng(9)

    def setup(N, M=6, R=3):
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)))
        dbs = [muse.DeviceBatch(eng, dg, rng.standard_normal(N)) for _ in range(R)]
        for db in dbs:
            db.scores()
        return dg, dbs

    dg, dbs = setup(1024)
    bands, signs = [(1, 7), (-7, -1), (-3, 3)], [0, 1, -1]
    muse.score_many_in_lag_bands(dbs, bands, signs)                  # (a mixed packed pass's scores to leave alone)
    assert all(eng.kernel_name(db).startswith("xcorr_window_many_each_mfma<2, ") for db in dbs)

    def i32(*v):
        return (ctypes.c_int32 * len(v))(*v)
    lo, hi, sg = i32(1, -7, -3), i32(7, -1, 3), i32(0, 1, -1)
    arr = (ctypes.c_void_p * 3)(dbs[0]._h, None, dbs[2]._h)          # NULL in the list
    before = state(eng, dbs)
    assert L.muse_batch_score_many_in_lag_bands(arr, 3, lo, hi, sg) == B.MUSE_ERR_INVALID
    arr = (ctypes.c_void_p * 3)(*[db._h for db in dbs])
    assert L.muse_batch_score_many_in_lag_bands(arr, 0, lo, hi, sg) == B.MUSE_ERR_INVALID
    assert L.muse_batch_score_many_in_lag_bands(arr, 3, None, hi, sg) == B.MUSE_ERR_INVALID
    assert L.muse_batch_score_many_in_lag_bands(arr, 3, lo, None, sg) == B.MUSE_ERR_INVALID
    for (s0, p0, k0, w0), (s1, p1, k1, w1) in zip(before, state(eng, dbs)):
        assert same_bits(s0, s1) and (p0, k0, w0) == (p1, k1, w1)
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands([dbs[0], dbs[1], dbs[0]], bands, signs), B.MUSE_ERR_INVALID)
    for k in range(3):                                               # lag_lo > lag_hi at one index (the C call: the mirror has its own check)
        bad_lo = i32(*[9 if r == k else v for r, v in enumerate(lo)])
        refused(muse, eng, dbs, lambda: B.check(L.muse_batch_score_many_in_lag_bands(arr, 3, bad_lo, hi, sg)), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.run_many_in_lag_bands(dbs, [(9, b[1]) if r == k else b for r, b in enumerate(bands)]), B.MUSE_ERR_INVALID)
        bad_sg = i32(*[2 if r == k else v for r, v in enumerate(sg)])  # sign 2 at one index
        refused(muse, eng, dbs, lambda: B.check(L.muse_batch_score_many_in_lag_bands(arr, 3, lo, hi, bad_sg)), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, bands, [2 if r == k else v for r, v in enumerate(signs)]), B.MUSE_ERR_INVALID)
        refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, [(513, 600) if r == k else b for r, b in enumerate(bands)], signs),
                B.MUSE_ERR_INVALID)                                  # nothing of one band is left at FFT length 1024
    tn, thr = i32(5, 3, 3), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o_s, o_l, o_v = (ctypes.c_int64 * 15)(), (ctypes.c_int32 * 15)(), (ctypes.c_double * 15)()
    cnt, mean = i32(0, 0, 0), (ctypes.c_double * 3)()
    refused(muse, eng, dbs, lambda: B.check(L.muse_batch_run_many_in_lag_bands(arr, 3, None, 0, lo, hi, tn, thr, sg, 1, 4, o_s, o_l, o_v, cnt, mean)),
            B.MUSE_ERR_INVALID)                                      # out_stride < top_n[0]
    refused(muse, eng, dbs, lambda: B.check(L.muse_batch_run_many_in_lag_bands(arr, 3, None, 0, lo, hi, None, thr, sg, 1, 5, o_s, o_l, o_v, cnt, mean)),
            B.MUSE_ERR_INVALID)
    refused(muse, eng, dbs, lambda: muse.run_many_in_lag_bands(dbs, bands, group_id=np.zeros(6, dtype=np.int32), G=-1, sign_filter=signs), B.MUSE_ERR_INVALID)
    dbs[1].set_lag_window(7)                                         # one member with a window of its own that differs from its band
    dbs[1].scores()
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, bands, signs), B.MUSE_ERR_INVALID)
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, [(1, 7), (-3, 3), (-7, 7)], signs), B.MUSE_ERR_INVALID)
    assert dbs[1].lag_window() == 7
    got = muse.scores_many_in_lag_bands(dbs, [(1, 7), (-7, 7), (-3, 3)], signs)      # equal to the call's: allowed, and left on
    assert dbs[1].lag_window() == 7 and np.all(np.abs(got[1][0]) <= 7)
    dbs[1].set_lag_window(-1)
    close(dbs, dg)
    dg, dbs = setup(100, R=2)                                        # an empty band at n = 128
    refused(muse, eng, dbs, lambda: muse.score_many_in_lag_bands(dbs, [(1, 7), (100, 226)], [0, 1]), B.MUSE_ERR_INVALID)
    close(dbs, dg)


# ------------------------------------------------------------------ 4. the Run form
@pytest.mark.parametrize("N", MB.RUN_NS)
def test_run_many_in_lag_bands_is_the_single_runs(muse, eng, oracle, N):
    """run_many_in_lag_bands with a band, a top_n, a threshold and a sign per reference, ungrouped and in label groups of three:
    the oracle's selection fed with the definition's per-series (lag, mv) of every reference (with room for every series: the rows
    hold the first reference and its negated copy, equal magnitudes, so at a top-N boundary the last bit decides which of the two
    stays), and each batch's own run_in_lag_band bit for bit under the per-reference top_n"""
    M, R = MB.RUN_M, len(MB.RUN_ASSIGN)
    ref, rows = LB.run_case(N)
    refs = MLR.make_refs(ref, N, 1000 + N)[:R]
    bands, signs = MB.bands_of(MB.RUN_ASSIGN), MB.signs_of(MB.RUN_ASSIGN)
    exps = []
    for r in range(R):
        e, n = LB.expect(oracle, refs[r], rows, (bands[r],), (signs[r],))
        exps.append(e[(bands[r][0], bands[r][1], signs[r])])
        assert not exps[r][2].any()
    G = M // MB.RUN_GROUP
    gid = (np.arange(M) % G).astype(np.int32)                        # (keeps rows 1 and 2 apart, as tests/test_gpu_many_lag_band.py does)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs, un = batches(muse, eng, dg, refs), batches(muse, eng, dg, refs)
    selected = 0
    for ab in (True, False):
        for g, Gn in ((None, 0), (gid, G)):
            full = muse.run_many_in_lag_bands(dbs, bands, g, Gn, M, MB.RUN_THRESHOLD, signs, ab)
            assert eng.kernel_name(dbs[0]).startswith("xcorr_window_many_each_mfma<4, ")
            got = muse.run_many_in_lag_bands(dbs, bands, g, Gn, MB.RUN_TOP_N, MB.RUN_THRESHOLD, signs, ab)
            for r in range(R):
                (lo, hi), s = bands[r], signs[r]
                L = max(abs(lo), abs(hi))
                _assert_run(full[r], oracle.results(exps[r][0], exps[r][1], g, Gn, ab, L, M, MB.RUN_THRESHOLD[r], s))
                one = un[r].run_in_lag_band(lo, hi, g, Gn, MB.RUN_TOP_N[r], MB.RUN_THRESHOLD[r], s, ab)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(got[r][:3], one[:3])), (N, r, ab, Gn)
                assert got[r][3] == one[3] or (np.isnan(got[r][3]) and np.isnan(one[3]))    # (an empty selection has no mean)
                assert len(got[r][0]) == min(MB.RUN_TOP_N[r], len(full[r][0]))
                assert dbs[r].last_run_path() == 0 and dbs[r].lag_window() == -1
                selected += len(got[r][0])
    assert selected > 60, selected
    close(dbs, un, dg)


# ------------------------------------------------------------------ 5. the label level
def test_label_level_honours_each_results(muse, eng, oracle):
    """RunManySigned over three batches whose Results differ in MaxLag, TopN, Threshold and SignFilter, and RunManyInLagBands /
    RunManySignedInLagBands with a band per batch: every Results.Fetch() is that of a twin batch run through its own method"""
    N, M = 480, MB.RUN_M
    ref, rows = LB.run_case(N)
    refs = MLR.make_refs(ref, N, 1000 + N)[:3]
    G = M // MB.RUN_GROUP
    labels = [{"trio": "t%02d" % (i % G), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    settings = ((7, 12, 0.0, muse.SignFilter_ANY), (3, 5, 0.1, muse.SignFilter_NEG), (15, 20, 0.05, muse.SignFilter_POS))
    bands = [b for b, _ in MB.RUN_ASSIGN]

    def make():
        res = [muse.NewResults(*st) for st in settings]
        return res, [muse.NewBatch(muse.NewSeries(refs[r], muse.NewLabels({"trio": "ref%d" % r})), comp, res[r], 8, engine=eng) for r in range(3)]

    def fetched(res):
        got, mean = res.Fetch()
        return [(int(sc.Labels.labels["i"]), sc.Lag, sc.PercentScore) for sc in got], mean

    fed = 0
    for by in (None, ["trio"]):
        for many, own in ((lambda bs: muse.RunManySigned(bs, by), lambda b, r: b.RunSigned(by)),
                          (lambda bs: muse.RunManySignedInLagBands(bs, by, bands), lambda b, r: b.RunSignedInLagBand(by, *bands[r])),
                          (lambda bs: muse.RunManyInLagBands(bs, by, bands), lambda b, r: b.RunInLagBand(by, *bands[r]))):
            res, bs = make()
            many(bs)
            res1, bs1 = make()
            for r in range(3):
                own(bs1[r], r)
                a, am = fetched(res[r])
                b, bm = fetched(res1[r])
                assert [(i, l) for i, l, _ in a] == [(i, l) for i, l, _ in b], (by, r)
                assert np.array([s for _, _, s in a]).tobytes() == np.array([s for _, _, s in b]).tobytes(), (by, r)
                assert am == bm or (np.isnan(am) and np.isnan(bm))
                fed += len(a)
    assert fed > 40, fed
