"""Many references inside a lag band or under a sign, in one pass over the rows (muse_batch_score_many_in_lag_band): the
many-references forms of DeviceBatch.score_in_lag_band / Batch.RunInLagBand / Batch.RunSignedInLagBand, on muse.py's shared
cores (_scores_many, _run_many, _run_many_labels).  One device."""
from . import binding as B
from . import muse as M


def _check(who, lag_lo, lag_hi, sign=0):
    if lag_lo > lag_hi:
        raise B.MuseError(B.MUSE_ERR_INVALID, "%s needs lagLo <= lagHi" % who)
    if sign not in (M.SignFilter_ANY, M.SignFilter_POS, M.SignFilter_NEG):
        raise B.MuseError(B.MUSE_ERR_INVALID, "%s needs a sign of -1, 0 or 1" % who)


def score_many_in_lag_band(batches, lag_lo, lag_hi, sign=0):
    """muse_batch_score_many_in_lag_band: R references against one resident group, each series' best match inside the lags
    lag_lo .. lag_hi, which need not hold lag 0 -- (1, k): "what led each reference by 1 .. k samples" -- by magnitude (sign = 0),
    its largest positive (+1) or most negative (-1) value; (lag 0, +0.0) where nothing wins.  One band and one sign for every
    reference, one pass over the rows: up to 48 lags the references' table rows packed into one matrix product per launch
    (asynchronous; results land in each DeviceBatch's own buffers, bit-identical to score_in_lag_band per batch on the direct
    product; no batch's own window changes).  sign = 0 with lag 0 inside is score_many_in_lag_range."""
    _check("score_many_in_lag_band", lag_lo, lag_hi, sign)
    batches, arr = M._batch_handles(batches)
    B.check(B.load().muse_batch_score_many_in_lag_band(arr, len(batches), int(lag_lo), int(lag_hi), int(sign)))


def scores_many_in_lag_band(batches, lag_lo, lag_hi, sign=0):
    """score_many_in_lag_band + copy back: list of (lag, mv), one per batch"""
    _check("scores_many_in_lag_band", lag_lo, lag_hi, sign)
    return M._scores_many("muse_batch_score_many_in_lag_band", batches, int(lag_lo), int(lag_hi), int(sign))


def run_many_in_lag_band(batches, lag_lo, lag_hi, group_id=None, G=0, top_n=20, threshold=0.0, sign_filter=0, abs_scores=True):
    """muse_batch_run_many_in_lag_band: DeviceBatch.run_in_lag_band for every reference (Results.MaxLag = max(|lag_lo|, |lag_hi|);
    sign_filter is the argmax's sign and the selection's filter); returns a list of (series, lag, score, mean_abs), one per batch"""
    _check("run_many_in_lag_band", lag_lo, lag_hi, sign_filter)
    return M._run_many("muse_batch_run_many_in_lag_band", batches, group_id, G, (lag_lo, lag_hi), top_n, threshold, sign_filter,
                       abs_scores)


def many_lag_band_plan(N, f32, lag_lo, lag_hi, sign, R):
    """muse_test_many_lag_band_plan (no device): MUSE_IN_WINDOW_* -- the pass score_many_in_lag_band takes for R references against
    series of N samples (f32: float32 storage) inside the lags lag_lo .. lag_hi under the sign; sign = 0 with lag 0 inside is
    many_lag_range_plan"""
    return M._plan_path("muse_test_many_lag_band_plan", N, bool(f32), lag_lo, lag_hi, sign, R)


def _run_many_band_labels(batches, groupByLabels, lagLo, lagHi, each, signed):
    """the feed of RunManyInLagBand / RunManySignedInLagBand: _run_many_labels with the (sign_filter, abs_scores) the batch's own
    method hands its device call -- (ANY, magnitudes) without a sign, (the shared Results.SignFilter, signed values) under one"""
    batches = list(batches)
    if batches and any(b._engines for b in batches):
        raise B.MuseError(B.MUSE_ERR_UNSUPPORTED, each + " runs on one device")
    sign = batches[0].Results.SignFilter if signed and batches else M.SignFilter_ANY
    _check(each, lagLo, lagHi, sign)

    def run(dbs, gid, G, _max_lag, top_n, threshold, _sign_filter, abs_scores=True):
        return run_many_in_lag_band(dbs, lagLo, lagHi, gid, G, top_n, threshold, sign, sign == M.SignFilter_ANY)
    single = "RunSignedInLagBand" if signed else "RunInLagBand"
    return M._run_many_labels(batches, groupByLabels, lambda b: getattr(b, single)(groupByLabels, lagLo, lagHi), run, False, "range")


def RunManyInLagBand(batches, groupByLabels, lagLo, lagHi):
    """RunMany inside the lag band lagLo .. lagHi, which need not hold lag 0 (muse_batch_run_many_in_lag_band): every batch receives
    what its own RunInLagBand(groupByLabels, lagLo, lagHi) gives -- the argmax by magnitude, the Results' own filters applied
    afterwards -- from one pass over the rows.  One device.  Batches that do not qualify for RunMany take RunInLagBand one after
    the other."""
    return _run_many_band_labels(batches, groupByLabels, lagLo, lagHi, "RunManyInLagBand", False)


def RunManySignedInLagBand(batches, groupByLabels, lagLo, lagHi):
    """RunManyInLagBand with the shared Results.SignFilter restricting the ARGMAX: every batch receives what its own
    RunSignedInLagBand(groupByLabels, lagLo, lagHi) gives; under a sign the Scores carry the signed value.  Batches whose Results
    settings differ take RunSignedInLagBand one after the other, each under its own SignFilter."""
    return _run_many_band_labels(batches, groupByLabels, lagLo, lagHi, "RunManySignedInLagBand", True)
