"""go-muse_amd: MI355X-native engine for go-muse's XCorr / Batch.Run hot path.

The directory name carries a hyphen (it mirrors the reference's name), so load
it with importlib.import_module("go-muse_amd").  Contents:
  csrc/      hand-written HIP kernels (gfx950) + the C-ABI implementation
  build.py   hipcc driver -> lib/libmuse_hip.so (in-tree)
  binding.py ctypes view of include/muse_hip.h
  muse.py    host-side mirror of the reference's Series/Group/Results/Batch API
  dist.py    one-process-per-GPU sharding + gather of per-shard top-N records
"""
from . import build  # noqa: F401
from . import binding  # noqa: F401
from .binding import MuseError  # noqa: F401
from . import dist  # noqa: F401
from .muse import (Batch, DefaultLabel, DeviceBatch, DeviceGroup, Engine, Group, Labels, Muse, New,  # noqa: F401
                   NewBatch, NewGroup, NewLabels, NewResults, NewSeries, Results, Score, Series,
                   SignFilter_ANY, SignFilter_NEG, SignFilter_POS, get_engine, merge_records, next_pow2,
                   RunMany, run_many, score_many, scores_many, xcorr_groups, device_count,
                   RunManyWindowed, run_many_windowed, score_many_windowed, scores_many_windowed, window_many_plan, window_rows_plan, in_window_plan,
                   RunManyInWindow, run_many_in_window, score_many_in_window, scores_many_in_window, many_in_window_plan,
                   slide_in_window_plan, lag_range_plan, signed_lag_range_plan, lag_band_plan, rows_lag_range_plan,
                   RunManyInLagRange, run_many_in_lag_range, score_many_in_lag_range, scores_many_in_lag_range, many_lag_range_plan,
                   window_many_plan_rows,
                   merge_group_records, merge_group_winners)
from . import many_band  # noqa: F401
from .many_band import (RunManyInLagBand, RunManySignedInLagBand, run_many_in_lag_band, score_many_in_lag_band,  # noqa: F401
                        scores_many_in_lag_band, many_lag_band_plan)
from . import many_bands  # noqa: F401
from .many_bands import (RunManyInLagBands, RunManySignedInLagBands, RunManySigned, run_many_in_lag_bands,  # noqa: F401
                         score_many_in_lag_bands, scores_many_in_lag_bands, many_lag_bands_plan)
# (the package attribute lag_profile is the module's row-level function of that name)
from .lag_profile import LagProfiles, lag_profile, lag_profile_into, lag_profile_plan  # noqa: F401
