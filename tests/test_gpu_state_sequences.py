"""GPU test of cross-feature invalidation (run with -m gpu on an MI355X): one long-lived resident group with two or three batches
taken through seeded random sequences of appends, staged commits, gathers, slides, fused slide-and-score calls, window settings,
screened and plain Runs, many-reference passes, cache builds and drops and Muse.Runs off a template.  A numpy model says what the rows
must be after every step; the CPU oracle, on the model's rows, is the expectation of every reading operation (tests/_seq.py: the
model, the generator, the runner and the rules of comparison; tests/test_state_sequences_cpu.py: what is asserted of the committed
seeds without a device).

State that outlives a call and that these sequences cross: the group's spectrum cache (zc_state, zc_rows, zc_rewrites, its segments),
the kept statistics of huge rows (hstats_rows), the rewrites counter, the staging pair, open staging windows and the gather's index
list; a batch's kernel-selection memory (handoff_M, handoff_rewrites), scores_exact / last_screened / costly_key of the
filter-and-refine Run, the score origin, the window setting and its table cache (lag_window, win_L), gid_valid; the context's pooled
Muse.Run slots and their window tables, the screening switch and the cache limits.

A failure prints the seed, the failing step and the operation list so far as a _seq.replay(...) call; MUSE_TEST_SEQ_SEED=<int> adds a
seed to every class.  MUSE_TEST_SEQ_TIMES=<file> appends every case's wall time (profiles/state_sequences.txt)."""
import os
import time

import pytest

import _seq
from _load import pkg

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


def _sequence(muse, eng, oracle, cls, seed):
    t0 = time.perf_counter()
    r = _seq.Runner(muse, eng, oracle, cls, seed)
    r.run()
    dt = time.perf_counter() - t0
    print("class %s seed %d: %d steps, %d rows at the end, %.2f s, kernels %s" % (cls, seed, len(r.ops), r.m.M, dt, sorted(r.kernels)))
    path = os.environ.get("MUSE_TEST_SEQ_TIMES")
    if path:
        with open(path, "a") as f:
            f.write("class %s seed %-4d N %-6d steps %-3d rows at the end %-5d wall %.2f s\n" % (cls, seed, r.m.shape.N, len(r.ops), r.m.M, dt))
    return r


CASES = [(cls, seed) for cls in _seq.CLASSES for seed in _seq.seeds_of(cls)]


@pytest.mark.parametrize("cls,seed", CASES)
def test_sequence(muse, eng, oracle, cls, seed):
    r = _sequence(muse, eng, oracle, cls, seed)
    # what the class is there to reach, in every sequence of it
    names = set(r.kernels) | ({"cache"} if r.cache_seen else set())
    want = dict(a=("xcorr_fused_n4096_fold", "xcorr_cached_n4096", "cache"), b=("xcorr_fused_small<9",), c=("xcorr_fused_small<11",),
                d=("xcorr_fused_real8k",), e=("xcorr_fused_small<9",), f=("huge_rows",), g=("xcorr_fused_n4096_fold", "xcorr_fused_n4096_occ4"))[cls]
    for w in want:
        assert any(x.startswith(w) for x in names), (cls, seed, w, sorted(names))
