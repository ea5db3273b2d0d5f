"""Lag profiles (muse_batch_lag_profile / muse_batch_lag_profile_device): the correlation of a resident group's series against a
batch's reference at every lag of lag_lo .. lag_hi -- the curve behind a (lag, score), where every scoring call returns its argmax
alone.  Row-level forms over a DeviceBatch, the planner, and the label-level form over a Batch.  One device."""
import ctypes

import numpy as np

from . import binding as B
from . import muse as M


def _series(series):
    """(the int64 index array to keep alive or None, its C pointer or NULL, K)"""
    if series is None:
        return None, None, 0
    idx = np.ascontiguousarray(series, dtype=np.int64).reshape(-1)
    return idx, B.i64ptr(idx), int(idx.shape[0])


def lag_profile(device_batch, lag_lo, lag_hi, series=None):
    """muse_batch_lag_profile: float64 [K or M, W], W = lag_hi - lag_lo + 1; out[k, v] = cc[(lag_lo + v) mod n] of series[k] (None:
    every series of the group in order) -- raw values, +0.0 for a series with sigma == 0, NaN for one that holds NaN or Inf.  Bit for
    bit what the band, range and signed passes scan at that lag on the direct product.  Any lags inside -(n / 2 - 1) .. n / 2, not
    clipped; float64 groups of up to 65536 samples.  The batch's scores stay as they were."""
    idx, ptr, K = _series(series)
    lag_lo, lag_hi = int(lag_lo), int(lag_hi)
    W = max(lag_hi - lag_lo + 1, 0)
    out = np.zeros((K if idx is not None else device_batch.dgroup.M, W))
    B.check(B.load().muse_batch_lag_profile(device_batch._h, ptr, K, lag_lo, lag_hi, B.dptr(out), W))
    return out


def lag_profile_into(device_batch, lag_lo, lag_hi, tensor, series=None):
    """muse_batch_lag_profile_device: fills a contiguous 2-D float64 torch tensor [K or M, W] on the batch's device, enqueued on the
    batch's stream like a score pass (asynchronous, and not ordered against torch's streams: what torch has enqueued on the tensor
    must have finished, and torch.cuda.synchronize() or the engine's comes before the tensor is read).  Returns the tensor.  A wrong
    dtype, device or shape is a MuseError(MUSE_ERR_INVALID) before any C call."""
    import torch
    idx, ptr, K = _series(series)
    lag_lo, lag_hi = int(lag_lo), int(lag_hi)
    rows = K if idx is not None else device_batch.dgroup.M
    W = lag_hi - lag_lo + 1
    if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float64:
        raise B.MuseError(B.MUSE_ERR_INVALID, "lag_profile_into needs a float64 torch tensor")
    if tensor.dim() != 2 or tuple(tensor.shape) != (rows, W) or not tensor.is_contiguous():
        raise B.MuseError(B.MUSE_ERR_INVALID, "lag_profile_into needs a contiguous tensor of shape [%d, %d], not %s"
                          % (rows, W, list(tensor.shape)))
    if tensor.device.type != "cuda" or tensor.device.index != device_batch.engine.device:
        raise B.MuseError(B.MUSE_ERR_INVALID, "lag_profile_into needs a tensor on the batch's device (cuda:%d), not %s"
                          % (device_batch.engine.device, tensor.device))
    B.check(B.load().muse_batch_lag_profile_device(device_batch._h, ptr, K, lag_lo, lag_hi, ctypes.c_void_p(tensor.data_ptr()), W))
    return tensor


def lag_profile_plan(N, lag_lo, lag_hi):
    """muse_test_lag_profile_plan (no device): [(first lag, table rows)] of the launches a profile of lag_lo .. lag_hi over series of N
    samples takes -- consecutive, at most 127 rows each"""
    n = ctypes.c_int32(0)
    lib = B.load()
    B.check(lib.muse_test_lag_profile_plan(int(N), int(lag_lo), int(lag_hi), ctypes.byref(n), None, None, 0))
    lo = np.zeros(max(n.value, 1), dtype=np.int32)
    rows = np.zeros(max(n.value, 1), dtype=np.int32)
    B.check(lib.muse_test_lag_profile_plan(int(N), int(lag_lo), int(lag_hi), ctypes.byref(n), B.i32ptr(lo), B.i32ptr(rows), n.value))
    return [(int(lo[j]), int(rows[j])) for j in range(n.value)]


def LagProfiles(batch, lagLo, lagHi, scores=None):
    """The curves behind a Batch's Scores: [(Score, lags[W], cc[W])] for every Score of `scores` (default: batch.Results.Fetch()[0],
    which empties the Results as Fetch does), cc the lag profile of the series of batch.Comparison that carries the Score's Labels
    (the first one, where several do).  A Score whose Labels are not in the group is a MuseError.  One device."""
    if batch._engines:
        raise B.MuseError(B.MUSE_ERR_UNSUPPORTED, "LagProfiles runs on one device: this batch is sharded over %d engines"
                          % len(batch._engines))
    if scores is None:
        scores = batch.Results.Fetch()[0]
    scores = list(scores)
    row_of = {}
    for i, s in enumerate(batch.Comparison._series_list()):
        row_of.setdefault(s.Labels().ID(), i)
    idx = []
    for sc in scores:
        key = sc.Labels.ID() if sc.Labels is not None else None
        if key not in row_of:
            raise B.MuseError(B.MUSE_ERR_INVALID, "LagProfiles: no series of the comparison group carries %r" % (sc.Labels,))
        idx.append(row_of[key])
    lags = np.arange(int(lagLo), int(lagHi) + 1, dtype=np.int64)
    if not idx:
        return []
    cc = lag_profile(batch._batch(), lagLo, lagHi, np.array(idx, dtype=np.int64))
    return [(sc, lags.copy(), cc[k].copy()) for k, sc in enumerate(scores)]
