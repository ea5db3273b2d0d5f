"""Inputs shared by tests/test_many_lag_bands_cpu.py and tests/test_gpu_many_lag_bands.py (muse_batch_score_many_in_lag_bands): the rows
and the first six references of tests/_manylagband.py's case(N), the named per-reference assignments of ((lo, hi), sign), the lists
the GPU test cuts and permutes from them, and the expectations -- per reference and row tests/_lagband.py's definition on the
oracle's correlation.  Nothing here touches the code under test: the CPU test checks, on exactly these (N, reference, band, sign)
tuples, that the oracle by itself flags no tie, so the GPU tests may demand exact lags on every row."""
import functools

import _lagband as LB
import _lagsweep as LS
import _manylagband as MLB

M = MLB.M
DIRECT_NS = MLB.DIRECT_NS
SMALL_MS = MLB.SMALL_MS
SMALL_M_N = MLB.SMALL_M_N
REFS = 6

# ((lo, hi), sign) per batch
MIXED = (((1, 7), 0), ((-7, -1), 1), ((1, 16), -1), ((-3, 12), 0), ((1, 1), 1), ((2, 18), 0))   # W = 7, 7, 16, 16, 1, 17: 64 rows, 4 tiles, one launch
SYMMETRIC = (((-7, 7), 0), ((-3, 3), -1), ((-15, 15), 1), ((-7, 0), 0))                            # different MaxLags and SignFilters: RunManySigned's
CUT = (((1, 48), 0), ((-48, -1), 1), ((1, 16), -1), ((5, 36), 0))                                  # 96 + 16 = 112 rows close launch 0; (5, 36) goes alone
ALONE = (((1, 7), 0), ((49, 97), 1), ((1, 8), -1))                                                 # W = 49 is never packed; 0 and 2 share a launch around it
FAR = (((200, 230), 1), ((-255, -200), 0), ((100, 226), -1))                                       # 31, 56 and 127 rows: every one alone; empty at n = 128
UNIFORM = (((1, 7), 1),) * 6                                                                       # delegates
ASSIGNMENTS = (("MIXED", MIXED), ("SYMMETRIC", SYMMETRIC), ("CUT", CUT), ("ALONE", ALONE), ("FAR", FAR), ("UNIFORM", UNIFORM))

# the launches of the named assignments at the FFT lengths that leave their bands whole: [(members, tiles, kc)] in launch order
LAUNCHES = {"MIXED": [((0, 1, 2, 3, 4, 5), 4, 512)],
            "SYMMETRIC": [((0, 1, 2, 3), 4, 1024)],
            "CUT": [((0, 1, 2), 7, 1024), ((3,), 2, 1024)],
            "ALONE": [((0, 2), 1, 1024), ((1,), 4, 1024)],
            "FAR": [((0,), 2, 1024), ((1,), 4, 1024), ((2,), 8, 1024)]}


def bands_of(assign):
    return [b for b, _ in assign]


def signs_of(assign):
    return [s for _, s in assign]


def lists(name, assign):
    """the lists the GPU test runs for an assignment: [(tag, reference indices, ((lo, hi), sign) per member)] -- the list as it is,
    reversed, rotated, and cut to R = 2 and 3 (reference r keeps its own series: what moves is its place and its question)"""
    R = len(assign)
    idx = list(range(R))
    out = [(name, idx, list(assign))]
    if name == "UNIFORM":
        return out
    out.append((name + " reversed", idx[::-1], list(assign)[::-1]))
    rot = idx[1:] + idx[:1]
    out.append((name + " rotated, other references", idx, [assign[k] for k in rot]))
    for cut in (2, 3):
        if cut < R:
            out.append((name + " R=%d" % cut, idx[:cut], list(assign)[:cut]))
            out.append((name + " last %d" % cut, idx[-cut:], list(assign)[-cut:]))
    return out


def all_lists():
    return [l for name, assign in ASSIGNMENTS for l in lists(name, assign)]


def tuples():
    """every (reference index, lo, hi, sign) the GPU test asks of case(N), the same for every N"""
    seen = set()
    for _, idx, assign in all_lists():
        for r, ((lo, hi), s) in zip(idx, assign):
            seen.add((r, lo, hi, s))
    return sorted(seen)


def case(N, m=M):
    """(ref, rows, the first six references of tests/_manylagband.py's case)"""
    ref, rows, refs = MLB.case(N, m)
    return ref, rows, refs[:REFS]


@functools.lru_cache(maxsize=None)
def _expect(oracle, N):
    ref, rows, refs = case(N)
    n = LS.fft_len(N)
    out = {}
    for r in range(REFS):
        mine = sorted({(lo, hi, s) for q, lo, hi, s in tuples() if q == r})
        by_sign = {}
        for lo, hi, s in mine:
            by_sign.setdefault(s, []).append((lo, hi))
        for s, bands in by_sign.items():
            exp, n2 = LB.expect(oracle, refs[r], rows, bands, (s,))
            assert n2 == n
            for (lo, hi, s2), v in exp.items():
                out[(r, lo, hi, s2)] = v
    return out, n


def expectations(oracle, N):
    """{(reference index, lo, hi, sign): (lag[M], mv[M], tie[M])} for every tuple whose band is not empty at this length, and n;
    computed once per N and shared (the callers leave it unchanged)"""
    return _expect(oracle, N)


# ---- the Run form
RUN_NS = LB.RUN_NS
RUN_M = LB.RUN_M
RUN_GROUP = LB.RUN_GROUP
RUN_ASSIGN = (((1, 15), 0), ((-20, -1), 1), ((-7, 7), -1))
RUN_TOP_N = (20, 7, 12)
RUN_THRESHOLD = (0.0, 0.2, 0.05)

# the reference off the direct product of the GPU test (N = 480, reference 1 of case(480)): 200 lags, the masked transform pass
WIDE_N, WIDE_REF, WIDE = 480, 1, ((1, 200), 1)
