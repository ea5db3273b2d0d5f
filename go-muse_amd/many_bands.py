"""Many references, each inside its own lag band and under its own sign, in one pass over the rows
(muse_batch_score_many_in_lag_bands): the forms of many_band.py with a (lagLo, lagHi) and a sign PER BATCH, on muse.py's shared
cores, and the label-level RunMany* forms that honour each batch's own Results.  One device."""
import ctypes

import numpy as np

from . import binding as B
from . import muse as M
from .many_band import _check


def _per_batch(who, what, value, R, dtype):
    """a scalar broadcast to every batch, or a sequence with one entry per batch"""
    if np.ndim(value) == 0:
        return np.full(R, value, dtype=dtype)
    a = np.ascontiguousarray(value, dtype=dtype)
    if a.shape != (R,):
        raise B.MuseError(B.MUSE_ERR_INVALID, "%s needs one %s per batch (or one for all)" % (who, what))
    return a


def _bands(who, bands, signs, R):
    """(lag_lo[R], lag_hi[R], sign[R]) as int32 arrays, checked as the C call checks them"""
    bands = [(int(lo), int(hi)) for lo, hi in bands]
    if len(bands) != R:
        raise B.MuseError(B.MUSE_ERR_INVALID, "%s needs one (lagLo, lagHi) per batch" % who)
    sign = _per_batch(who, "sign", 0 if signs is None else signs, R, np.int64)
    for (lo, hi), s in zip(bands, sign):
        _check(who, lo, hi, int(s))
    lo = np.array([b[0] for b in bands], dtype=np.int32)
    hi = np.array([b[1] for b in bands], dtype=np.int32)
    return lo, hi, sign.astype(np.int32)


def score_many_in_lag_bands(batches, bands, signs=None):
    """muse_batch_score_many_in_lag_bands: R references against one resident group, batch r's best match per series inside its OWN
    lags bands[r] = (lo, hi) under its OWN sign signs[r] (a scalar: one sign for all; None: by magnitude) -- every batch is left as
    its own score_in_lag_band(lo, hi, sign) leaves it, bit for bit on the direct product, from one read of the rows: up to 48 lags
    per reference the references' table rows are packed into the tiles of one matrix product per launch, whatever their bands and
    signs (asynchronous; results land in each DeviceBatch's own buffers; no batch's own window changes).  One (lo, hi, sign) for
    the whole list is score_many_in_lag_band."""
    batches = list(batches)
    lo, hi, sign = _bands("score_many_in_lag_bands", bands, signs, len(batches))
    batches, arr = M._batch_handles(batches)
    B.check(B.load().muse_batch_score_many_in_lag_bands(arr, len(batches), B.i32ptr(lo), B.i32ptr(hi), B.i32ptr(sign)))


def scores_many_in_lag_bands(batches, bands, signs=None):
    """score_many_in_lag_bands + copy back: list of (lag, mv), one per batch"""
    batches = list(batches)
    lo, hi, sign = _bands("scores_many_in_lag_bands", bands, signs, len(batches))
    return M._scores_many("muse_batch_score_many_in_lag_bands", batches, B.i32ptr(lo), B.i32ptr(hi), B.i32ptr(sign))


def run_many_in_lag_bands(batches, bands, group_id=None, G=0, top_n=20, threshold=0.0, sign_filter=0, abs_scores=True):
    """muse_batch_run_many_in_lag_bands: DeviceBatch.run_in_lag_band(*bands[r], ...) for every reference, with its own top_n,
    threshold and sign_filter (scalars broadcast, sequences are per batch; sign_filter is the argmax's sign and the selection's
    filter; Results.MaxLag = max(|lo|, |hi|) per batch); returns a list of (series, lag, score, mean_abs), one per batch"""
    batches = list(batches)
    R = len(batches)
    who = "run_many_in_lag_bands"
    lo, hi, sign = _bands(who, bands, sign_filter, R)
    tn = _per_batch(who, "top_n", top_n, R, np.int32)
    thr = _per_batch(who, "threshold", threshold, R, np.float64)
    batches, arr = M._batch_handles(batches)
    cap = max(int(tn.max()), 1)
    o_s = np.zeros(R * cap, dtype=np.int64)
    o_l = np.zeros(R * cap, dtype=np.int32)
    o_v = np.zeros(R * cap)
    cnt = np.zeros(R, dtype=np.int32)
    mean = np.zeros(R)
    gid, gptr = M._gid_ptr(group_id)
    B.check(B.load().muse_batch_run_many_in_lag_bands(
        arr, R, gptr, int(G), B.i32ptr(lo), B.i32ptr(hi), B.i32ptr(tn), B.dptr(thr), B.i32ptr(sign), 1 if abs_scores else 0, cap,
        B.i64ptr(o_s), B.i32ptr(o_l), B.dptr(o_v), B.i32ptr(cnt), B.dptr(mean)))
    res = []
    for r in range(R):
        c = int(cnt[r])
        res.append((o_s[r * cap:r * cap + c].copy(), o_l[r * cap:r * cap + c].copy(), o_v[r * cap:r * cap + c].copy(), float(mean[r])))
    return res


def many_lag_bands_plan(N, f32, bands, signs=None):
    """muse_test_many_lag_bands_plan (no device): how score_many_in_lag_bands serves a list that does not share one (lo, hi, sign) --
    dict(path[R]: the MUSE_IN_WINDOW_* value of each reference's single dispatch; launches; launch_of[R]: the launch of a reference
    on the direct product, -1 otherwise; tiles_of[launches]; kc_of[launches]; img0[R]: the LDS offset of its staged image)"""
    bands = list(bands)
    R = len(bands)
    lo, hi, sign = _bands("many_lag_bands_plan", bands, signs, R)
    n = ctypes.c_int32(0)
    path, of, tiles, kc, img0 = (np.zeros(max(R, 1), dtype=np.int32) for _ in range(5))
    B.check(B.load().muse_test_many_lag_bands_plan(int(N), 1 if f32 else 0, R, B.i32ptr(lo), B.i32ptr(hi), B.i32ptr(sign), B.i32ptr(path),
                                                   B.i32ptr(of), ctypes.byref(n), B.i32ptr(tiles), B.i32ptr(kc), B.i32ptr(img0)))
    k = int(n.value)
    return dict(path=path[:R].copy(), launches=k, launch_of=of[:R].copy(), tiles_of=tiles[:k].copy(), kc_of=kc[:k].copy(),
                img0=img0[:R].copy())


def _run_many_bands_labels(batches, groupByLabels, bands, who, signed):
    """the feed of RunManyInLagBands / RunManySignedInLagBands: every batch's Results fed in group order what its own single method
    (RunInLagBand / RunSignedInLagBand, Batch._feed_in_window) feeds it -- up to EXACT_FEED_MAX_GROUPS label groups every group's
    winner, beyond the device's pre-selection under the batch's own TopN and Threshold -- with the (sign_filter, abs_scores) that
    method hands its device call: (ANY, magnitudes) without a sign, (the batch's own Results.SignFilter, signed values) under one.
    The C call takes one abs_scores: under signs the batches that report magnitudes (SignFilter_ANY) and those that report signed
    values take one pass each."""
    batches = list(batches)
    if not batches:
        return None
    bands = [(int(lo), int(hi)) for lo, hi in bands]
    if len(bands) != len(batches):
        raise B.MuseError(B.MUSE_ERR_INVALID, "%s needs one (lagLo, lagHi) per batch" % who)
    if any(b._engines for b in batches):
        raise B.MuseError(B.MUSE_ERR_UNSUPPORTED, who + " runs on one device")
    signs = [b.Results.SignFilter if signed else M.SignFilter_ANY for b in batches]
    for (lo, hi), s in zip(bands, signs):
        _check(who, lo, hi, s)
    b0 = batches[0]
    single = "RunSignedInLagBand" if signed else "RunInLagBand"
    if not all(b.Comparison is b0.Comparison and b._engine is b0._engine for b in batches):
        for b, (lo, hi) in zip(batches, bands):   # (no shared rows to read once: the single methods one after the other)
            getattr(b, single)(groupByLabels, lo, hi)
        return None
    comp = b0.Comparison
    labelValuesSet = comp.indexLabelValues(groupByLabels)
    if not labelValuesSet:
        return None
    series = comp._series_list()
    gid = comp._group_ids()
    G = len(labelValuesSet)
    for magnitudes in (True, False):
        idx = [r for r, s in enumerate(signs) if (s == M.SignFilter_ANY) == magnitudes]
        if not idx:
            continue
        dbs = [batches[r]._batch() for r in idx]
        if G <= M.EXACT_FEED_MAX_GROUPS:   # (as RunInWindow: one Score per group in group order through Results.Update)
            top_n, threshold = G, 0.0
        else:
            top_n, threshold = [batches[r].Results.TopN for r in idx], [batches[r].Results.Threshold for r in idx]
        res = run_many_in_lag_bands(dbs, [bands[r] for r in idx], gid, G, top_n, threshold, [signs[r] for r in idx], magnitudes)
        for r, (i, lag, score, _) in zip(idx, res):
            M._feed_in_group_order(batches[r].Results, series, gid, i, lag, score)
    return None


def RunManyInLagBands(batches, groupByLabels, bands):
    """RunMany with a lag band PER BATCH (muse_batch_run_many_in_lag_bands): batch r receives what its own
    RunInLagBand(groupByLabels, *bands[r]) gives -- the argmax by magnitude, its own Results' filters applied afterwards -- from one
    pass over the rows.  The batches' Results may differ in every field.  One device.  Batches that do not share the Comparison and
    the engine take RunInLagBand one after the other."""
    return _run_many_bands_labels(batches, groupByLabels, bands, "RunManyInLagBands", False)


def RunManySignedInLagBands(batches, groupByLabels, bands):
    """RunManyInLagBands with each batch's OWN Results.SignFilter restricting its argmax: batch r receives what its own
    RunSignedInLagBand(groupByLabels, *bands[r]) gives; under a sign the Scores carry the signed value."""
    return _run_many_bands_labels(batches, groupByLabels, bands, "RunManySignedInLagBands", True)


def RunManySigned(batches, groupByLabels):
    """RunManySignedInLagBands with bands[r] = (-MaxLag_r, MaxLag_r): every batch receives what its own RunSigned(groupByLabels)
    gives, under its own Results.MaxLag, TopN, Threshold and SignFilter, from one pass over the rows."""
    batches = list(batches)
    if any(b.Results.MaxLag < 0 for b in batches):
        raise B.MuseError(B.MUSE_ERR_INVALID, "RunManySigned needs Results.MaxLag >= 0")
    return _run_many_bands_labels(batches, groupByLabels, [(-b.Results.MaxLag, b.Results.MaxLag) for b in batches], "RunManySigned", True)
